"""Times the layer warp and the sampling maps at 1080p beside the renderer they share a chain with, in one GPU process:

  vm_render_layers_dev, 1 and 4 channels     device events around the kernel
  vm_frame_sampling_maps, all four outputs   wall clock of the whole call (kernel + 43.5 MB over the link, drained);
                                             flags only (2 MB over the link) as the closest view of the kernel alone
  vm_render_halfway_dev                      the yardstick: same frame, same process, device events
  download_v (+ download_qpath) + the numpy statement of tests/warp_ref.py: the route a host had before

with and without a path.  A warm-up of every call, then `--reps` rounds in which the device calls alternate; medians
and minima.  The maps of the last round are compared with the statement bit for bit (what was timed is what is
specified).  Writes a markdown note (default: profiles/layer_warp.md).  Development tool: the numbers gate nothing.

  python tools/dev_layer_warp.py [--out PATH] [--reps N] [--size WxH]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import warp_ref as R  # noqa: E402
from videomorphing_amd import capi, morph, synth  # noqa: E402

f32 = np.float32


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_warp.md"))
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
    fr = morph.Frame(ctx, w, h, ex)
    geo, col = 0.35, 0.35
    rows = []
    for with_path in (False, True):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u if with_path else None)
        t = {k: [] for k in ("render", "layers1", "layers4", "maps", "flags")}
        flags_only = np.empty((h, w), np.uint8)
        for rep in range(a.reps + 2):                               # two rounds of warm-up
            got = {"render": fr.render_halfway_dev(col, geo, 1)}
            for c in (1, 4):
                fr.upload_layers(*layers[c])
                fr.render_layers_dev(col, geo, 1)                   # (the first launch after an upload is not the timed one)
                got["layers%d" % c] = fr.render_layers_dev(col, geo, 1)
            maps = [None]
            got["maps"] = wall_ms(lambda: maps.__setitem__(0, fr.sampling_maps(geo)))
            got["flags"] = wall_ms(lambda: capi.check(fr._L.vm_frame_sampling_maps(fr._h, geo, None, None, None, flags_only.ctypes.data)))
            if rep >= 2:
                for k in t:
                    t[k].append(got[k])
        host = [None]
        t_host = wall_ms(lambda: host.__setitem__(0, R.sampling_maps(fr.download_v(), fr.download_qpath() if with_path else None, geo)))
        for g, r in zip(maps[0], host[0]):
            assert np.array_equal(g.view(np.uint32) if g.dtype == f32 else g, r.view(np.uint32) if r.dtype == f32 else r)
        assert np.array_equal(flags_only, host[0][3])
        rows.append((with_path, {k: (float(np.median(x)), float(np.min(x))) for k, x in t.items()}, t_host,
                     float(host[0][2].max()), float((host[0][3] != 3).mean())))
    px = w * h
    lines = [
        "# Layer warp and sampling maps at %dx%d beside the renderer" % (w, h),
        "",
        "Measured by `tools/dev_layer_warp.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the device" % (name, cus, a.reps),
        "calls alternating within a round.  Field: the synthetic ground-truth displacement (up to %.0f px) plus 0.05 px of noise;" % np.abs(d).max(),
        "path: a quarter of it, transposed; geo_fa = color_fa = %.2f, color_from 1.  `vm_render_halfway_dev` is the kernel" % geo,
        "this change leaves as it was: the yardstick.  Kernel columns are device events (`*_dev`), median (minimum); the",
        "maps call has no `_dev` form and is the wall clock of the whole call, drained.  The numbers gate nothing.",
        "",
        "| path | `vm_render_halfway_dev`, ms | `vm_render_layers_dev` 1 ch, ms | 4 ch, ms | `vm_frame_sampling_maps` all four, whole call, ms | flags only, whole call, ms | host route (`download_v` + numpy statement), ms |",
        "|---|---|---|---|---|---|---|",
    ]
    for with_path, t, t_host, resid, outside in rows:
        lines.append("| %s | %.4f (%.4f) | %.4f (%.4f) | %.4f (%.4f) | %.3f (%.3f) | %.3f (%.3f) | %.0f |" % (
            ("yes" if with_path else "no",) + t["render"] + t["layers1"] + t["layers4"] + t["maps"] + t["flags"] + (t_host,)))
    lines += [
        "",
        "Counted traffic per pixel (DESIGN.md 3.9): every kernel stages 3.8 cells of v (and u) of 8 B and walks 21 dependent",
        "taps from LDS; the renderer then gathers 2 x 4 RGBA8 texels and stores 3 B (11 B compulsory), the maps kernel stores",
        "21 B (%.1f MB per frame, all of which then crosses the link: the all-four column is that copy), the layer kernel" % (21 * px / 1e6),
        "gathers 2 x 4 texels of 4 C bytes and stores 4 C bytes (12 C B compulsory: %.1f MB per frame at 4 channels)." % (48 * px / 1e6),
        "Expectation from DESIGN.md 3.3: the chain dominates, so the layer kernels land near the renderer, the 4-channel one",
        "above the 1-channel one by its 16-byte gathers; whether it passes the renderer depends on what the renderer's own tail",
        "(byte unpacking, the double-precision rounding, three byte stores per pixel) costs.  Seen:",
        "",
    ]
    for with_path, t, t_host, resid, outside in rows:
        lines.append("%s path: 1 ch / renderer = %.2f, 4 ch / renderer = %.2f, flags-only call / renderer = %.2f; largest resid %.3g px, %.2f %% of pixels sample outside an image." % (
            "With a" if with_path else "Without a", t["layers1"][0] / t["render"][0], t["layers4"][0] / t["render"][0], t["flags"][0] / t["render"][0], resid, 100 * outside))
    lines += ["", "The all-four maps call is the link's: %.1f MB in %.3f ms = %.0f GB/s device to host, kernel included." % (
        21 * px / 1e6, rows[0][1]["maps"][0], 21 * px / 1e6 / rows[0][1]["maps"][0]), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
