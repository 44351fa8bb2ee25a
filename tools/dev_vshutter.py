"""Times the viewport calls over a shutter at 1080p beside the calls they compose, in one GPU process (RGB8 tail, T = 16
time samples, a shutter 0.45 .. 0.55, the colour at 0.5, linear ease, videomorphing_amd.transition.wipe's default schedule
on both planes):

  1  the identity viewport                     beside vm_render_shutter_dev and vm_render_transition_shutter_dev: what the
                                               composition costs when it composes nothing
  2  native scale with 2 x 2 sub-samples       beside sixteen vm_render_viewport_dev calls of 2 x 2 at the shutter's sample
                                               times (uniform family) and beside four times the 1 x 1 call of (1) (both
                                               families): whether sharing a staged window across sub-samples pays
  3  a half-size proxy of 2 x 2 x 16 and a quarter-size window of a 2.5x zoom at T = 16, each with its download
     (wall-clock), beside the host routes: sixteen vm_render_viewport calls, their downloads and a float mean in numpy
     (uniform); a full-size vm_render_transition_shutter, its download and a resample in numpy (scheduled: a 2 x 2 box mean;
     a bilinear gather)

with and without a path, device events around each call of 1 and 2.  The field is that of tools/dev_layer_warp.py
(profiles/layer_warp.md).  Two rounds of warm-up, then `--reps` rounds in which the compared calls alternate; medians, and
the minimum and maximum of the calls that exist already (their run-to-run spread is the yardstick).  The identity viewport
is compared byte for byte with both shutter calls before anything is timed.  Writes a markdown note (default:
profiles/viewport_shutter.md); `--label` names the build in it and `--append` adds the run as a further section.
Development tool: the numbers gate nothing.

  python tools/dev_vshutter.py [--out PATH] [--reps N] [--host-reps N] [--size WxH] [--label TEXT] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import shutter_ref  # noqa: E402
from dev_viewport import bilinear, box2, stat  # noqa: E402
from videomorphing_amd import capi, morph, synth, transition  # noqa: E402
from videomorphing_amd.viewport import Viewport  # noqa: E402

f32 = np.float32
FA, OPEN, CLOSE, T = 0.5, 0.45, 0.55, 16
EASE = capi.EASE_LINEAR


def float_mean(images):
    """the host's shutter: the float32 mean of rounded frames, rounded again"""
    acc = np.zeros(images[0].shape, f32)
    for im in images:
        acc += im
    return (acc / f32(len(images)) + f32(0.5)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewport_shutter.md"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=5)
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
    wipe = transition.wipe(w, h)
    ident = Viewport.identity(w, h)
    ss = ident.supersampled(2)
    proxy = Viewport.fit(w, h, w // 2, h // 2).supersampled(2)
    zoom = Viewport.zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 2.5, w // 4, h // 4)
    times = [float(t) for t in shutter_ref.sample_times(OPEN, CLOSE, T)]
    fr = morph.Frame(ctx, w, h, ex)
    dev_rows, host_rows = [], []
    for with_path in (False, True):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u if with_path else None)
        fr.upload_schedule(wipe, wipe)
        assert np.array_equal(fr.render_viewport_shutter(ident, FA, OPEN, CLOSE, T, 1), fr.render_shutter(FA, OPEN, CLOSE, T, 1))
        assert np.array_equal(fr.render_viewport_transition_shutter(ident, OPEN, CLOSE, T, FA, EASE, 1),
                              fr.render_transition_shutter(OPEN, CLOSE, T, FA, EASE, 1))
        ts = {}
        for rep in range(a.reps + 2):                               # two rounds of warm-up
            got = {
                "sh": fr.render_shutter_dev(FA, OPEN, CLOSE, T, 1),
                "vsh": fr.render_viewport_shutter_dev(ident, FA, OPEN, CLOSE, T, 1),
                "tsh": fr.render_transition_shutter_dev(OPEN, CLOSE, T, FA, EASE, 1),
                "vtsh": fr.render_viewport_transition_shutter_dev(ident, OPEN, CLOSE, T, FA, EASE, 1),
                "vsh4": fr.render_viewport_shutter_dev(ss, FA, OPEN, CLOSE, T, 1),
                "vp4x16": sum(fr.render_viewport_dev(ss, FA, t, 1) for t in times),
                "vtsh4": fr.render_viewport_transition_shutter_dev(ss, OPEN, CLOSE, T, FA, EASE, 1),
                "proxy_u": fr.render_viewport_shutter_dev(proxy, FA, OPEN, CLOSE, T, 1),
                "proxy_s": fr.render_viewport_transition_shutter_dev(proxy, OPEN, CLOSE, T, FA, EASE, 1),
                "zoom_u": fr.render_viewport_shutter_dev(zoom, FA, OPEN, CLOSE, T, 1),
                "zoom_s": fr.render_viewport_transition_shutter_dev(zoom, OPEN, CLOSE, T, FA, EASE, 1),
            }
            if rep >= 2:
                for k, t in got.items():
                    ts.setdefault(k, []).append(t)
        dev_rows.append((with_path, {k: stat(x) for k, x in ts.items()}))
        # with the download, wall-clock, beside the host routes
        keys = ("proxy_u", "proxy_u_host", "zoom_u", "zoom_u_host", "proxy_s", "proxy_s_host", "zoom_s", "zoom_s_host")
        wall = {k: [] for k in keys}
        for _ in range(a.host_reps + 1):
            c = [time.perf_counter()]
            pu = fr.render_viewport_shutter(proxy, FA, OPEN, CLOSE, T, 1); c.append(time.perf_counter())
            puh = float_mean([fr.render_viewport(proxy, FA, t, 1) for t in times]); c.append(time.perf_counter())
            zu = fr.render_viewport_shutter(zoom, FA, OPEN, CLOSE, T, 1); c.append(time.perf_counter())
            zuh = float_mean([fr.render_viewport(zoom, FA, t, 1) for t in times]); c.append(time.perf_counter())
            ps = fr.render_viewport_transition_shutter(proxy, OPEN, CLOSE, T, FA, EASE, 1); c.append(time.perf_counter())
            psh = box2(fr.render_transition_shutter(OPEN, CLOSE, T, FA, EASE, 1)); c.append(time.perf_counter())
            zs = fr.render_viewport_transition_shutter(zoom, OPEN, CLOSE, T, FA, EASE, 1); c.append(time.perf_counter())
            zsh = bilinear(fr.render_transition_shutter(OPEN, CLOSE, T, FA, EASE, 1), zoom); c.append(time.perf_counter())
            for k, t in zip(keys, np.diff(c)):
                wall[k].append(1e3 * t)
        off = tuple(int(np.abs(x.astype(int) - y.astype(int)).max()) for x, y in ((pu, puh), (zu, zuh), (ps, psh), (zs, zsh)))
        host_rows.append((with_path, {k: float(np.median(x[1:])) for k, x in wall.items()}, off))
    lines = [
        "%s The viewport calls over a shutter at %dx%d beside the calls they compose: %s" % ("##" if a.append else "#", w, h, a.label),
        "",
        "Measured by `tools/dev_vshutter.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the calls alternating" % (name.strip(), cus, a.reps),
        "within a round.  Field and path: those of `profiles/layer_warp.md`; the schedule is `transition.wipe`'s default on both",
        "planes.  RGB8, T = %d, shutter %.2f .. %.2f, colour at %.1f, linear ease, color_from 1.  Device events around each call, ms:" % (T, OPEN, CLOSE, FA),
        "median (minimum .. maximum over the rounds).  The numbers gate nothing.",
        "",
        "### 1: the identity viewport beside the shutter calls",
        "",
        "| path | vm_render_shutter | viewport, uniform | ratio | vm_render_transition_shutter | viewport, scheduled | ratio |",
        "|---|---|---|---|---|---|---|",
    ]
    for with_path, s in dev_rows:
        lines.append("| %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.3f | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.3f |"
                     % (("yes" if with_path else "no",) + s["sh"] + s["vsh"] + (s["vsh"][0] / s["sh"][0],) + s["tsh"] + s["vtsh"]
                        + (s["vtsh"][0] / s["tsh"][0],)))
    lines += [
        "",
        "### 2: native scale, 2 x 2 sub-samples",
        "",
        "| path | uniform 2 x 2 x 16 | 16 x vm_render_viewport of 2 x 2 | ratio | / (4 x the 1 x 1 call) | scheduled 2 x 2 x 16 | / (4 x the 1 x 1 call) |",
        "|---|---|---|---|---|---|---|",
    ]
    for with_path, s in dev_rows:
        lines.append("| %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.3f | %.3f | %.4f (%.4f .. %.4f) | %.3f |"
                     % (("yes" if with_path else "no",) + s["vsh4"] + s["vp4x16"] + (s["vsh4"][0] / s["vp4x16"][0], s["vsh4"][0] / (4 * s["vsh"][0]))
                        + s["vtsh4"] + (s["vtsh4"][0] / (4 * s["vtsh"][0]),)))
    lines += [
        "",
        "### 3: a %dx%d proxy of 2 x 2 x 16 (steps 2: the plain form) and a %dx%d window of a 2.5x zoom at T = 16" % (proxy.out_w, proxy.out_h, zoom.out_w, zoom.out_h),
        "",
        "Device ms as above; with the download, wall-clock ms, median of %d, beside the host route -- uniform: sixteen" % a.host_reps,
        "`vm_render_viewport` calls, their downloads and a float mean in numpy; scheduled: a full-size `vm_render_transition_shutter`,",
        "its download and a resample in numpy (a 2 x 2 box mean of the bytes; a bilinear gather of the bytes).  `off`: the largest",
        "difference of the two pictures in grey levels (the host routes round every sample or the whole frame to bytes first).",
        "",
        "| path | family | proxy, device | proxy + download | host route | off | zoom, device | zoom + download | host route | off |",
        "|---|---|---|---|---|---|---|---|---|---|",
    ]
    for (with_path, s), (_, wl, off) in zip(dev_rows, host_rows):
        for fam, k, o in (("uniform", "u", off[:2]), ("scheduled", "s", off[2:])):
            lines.append("| %s | %s | %.4f (%.4f .. %.4f) | %.2f | %.2f | %d | %.4f (%.4f .. %.4f) | %.2f | %.2f | %d |"
                         % (("yes" if with_path else "no", fam) + s["proxy_" + k] + (wl["proxy_" + k], wl["proxy_%s_host" % k], o[0])
                            + s["zoom_" + k] + (wl["zoom_" + k], wl["zoom_%s_host" % k], o[1])))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + "\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
