"""Times the filtered viewport calls at 1080p beside the bilinear viewport calls, in one GPU process:

  identity   the identity viewport, one sample
  zoom       the 480 x 270 window of a 2.5x zoom
  proxy      the 960 x 540 proxy of 2 x 2 samples (steps 2: the plain form)
  4 x 4      4 x 4 samples at native scale

each as RGB8 and as layers of 1 and 4 channels, with and without a path: vm_render_viewport[_layers]_dev beside
vm_frame_render_viewport_filtered[_layers]_dev under Catmull-Rom, Mitchell and the cubic B-spline (one kernel, three sets of
coefficients), device events around each call.  The field is that of tools/dev_viewport.py.  Two rounds of warm-up, then
`--reps` rounds in which the calls alternate; medians, and each cubic call's ratio to the bilinear one.  The bilinear
filter is compared byte for byte with vm_render_viewport before anything is timed.  Under `rocprofv3 --kernel-trace --stats`
the same run gives the kernels' medians side by side in one trace (k_viewport* and k_fview*).  Writes a markdown note
(default: profiles/filtered.md); `--label` names the build in it and `--append` adds the run as a further section.
Development tool: the numbers gate nothing.

  python tools/dev_filtered.py [--out PATH] [--reps N] [--size WxH] [--label TEXT] [--append]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from videomorphing_amd import capi, morph, synth  # noqa: E402
from videomorphing_amd.viewport import Viewport  # noqa: E402

f32 = np.float32
FA = 0.5
FILTERS = (("Catmull-Rom", capi.FILTER_CATMULL_ROM), ("Mitchell", capi.FILTER_MITCHELL), ("B-spline", capi.FILTER_BSPLINE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered.md"))
    ap.add_argument("--reps", type=int, default=15)
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
    views = (("identity", Viewport.identity(w, h)),
             ("zoom", Viewport.zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 2.5, w // 4, h // 4)),
             ("proxy", Viewport.fit(w, h, w // 2, h // 2).supersampled(2)),
             ("4 x 4", Viewport.identity(w, h).supersampled(4)))
    fr = morph.Frame(ctx, w, h, ex)
    rows = []
    for with_path in (False, True):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u if with_path else None)
        for _, vp in views[:2]:
            assert np.array_equal(fr.render_viewport_filtered(vp, capi.FILTER_BILINEAR, FA, FA, 1), fr.render_viewport(vp, FA, FA, 1))
        ts = {}
        for rep in range(a.reps + 2):                               # two rounds of warm-up
            got = {}
            for vn, vp in views:
                got[(vn, "RGB8", "bilinear")] = fr.render_viewport_dev(vp, FA, FA, 1)
                for fn, filt in FILTERS:
                    got[(vn, "RGB8", fn)] = fr.render_viewport_filtered_dev(vp, filt, FA, FA, 1)
            for ch in (1, 4):
                fr.upload_layers(*layers[ch])
                fr.render_layers_dev(FA, FA, 1)                     # (the first launch after an upload is not the timed one)
                for vn, vp in views:
                    got[(vn, "%d ch" % ch, "bilinear")] = fr.render_viewport_layers_dev(vp, FA, FA, 1)
                    for fn, filt in FILTERS:
                        got[(vn, "%d ch" % ch, fn)] = fr.render_viewport_filtered_layers_dev(vp, filt, FA, FA, 1)
            if rep >= 2:
                for k, t in got.items():
                    ts.setdefault(k, []).append(t)
        rows.append((with_path, {k: float(np.median(x)) for k, x in ts.items()}))
    lines = [
        "%s The filtered viewport calls at %dx%d beside the bilinear ones: %s" % ("##" if a.append else "#", w, h, a.label),
        "",
        "Measured by `tools/dev_filtered.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the calls alternating" % (name.strip(), cus, a.reps),
        "within a round.  Field and path: those of `profiles/viewport.md`.  color_fa = geo_fa = %.1f, color_from 1.  Device events" % FA,
        "around each call, ms, medians; `x`: the cubic call over the bilinear one.  The numbers gate nothing.",
        "",
        "| viewport | path | tail | bilinear | Catmull-Rom | x | Mitchell | x | B-spline | x |",
        "|---|---|---|---|---|---|---|---|---|---|",
    ]
    for vn, _ in views:
        for with_path, ts in rows:
            for tail in ("RGB8", "1 ch", "4 ch"):
                b = ts[(vn, tail, "bilinear")]
                cells = "".join(" %.4f | %.2f |" % (ts[(vn, tail, fn)], ts[(vn, tail, fn)] / b) for fn, _ in FILTERS)
                lines.append("| %s | %s | %s | %.4f |%s" % (vn, "yes" if with_path else "no", tail, b, cells))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + "\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
