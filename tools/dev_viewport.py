"""Times the viewport calls at 1080p beside what they replace, in one GPU process:

  1  the identity viewport, one sample        beside vm_render_halfway_dev and vm_render_layers_dev (1, 3, 4 channels)
  2  2 x 2 and 4 x 4 samples at native scale  beside N times (1): the window is staged once, whatever N is
  3  a half-size proxy of 2 x 2 samples and a 480 x 270 window of a 2.5x zoom, each with its download (wall-clock),
     beside the route they replace: vm_render_halfway, its download and a resample in numpy (a 2 x 2 box mean; a bilinear
     gather)
  4  the half-size proxy on the device (the plain form: its steps are above 1), the figure a larger-window class for
     1 < step <= 2 would have to beat

with and without a path, device events around each call of 1, 2 and 4.  The field is that of tools/dev_layer_warp.py
(profiles/layer_warp.md).  Two rounds of warm-up, then `--reps` rounds in which the calls alternate; medians, and the minimum
and maximum of the uniform calls (their run-to-run spread is the yardstick).  The identity viewport is compared byte for
byte with vm_render_halfway before anything is timed.  Writes a markdown note (default: profiles/viewport.md); `--label`
names the build in it and `--append` adds the run as a further section.  Development tool: the numbers gate nothing.

  python tools/dev_viewport.py [--out PATH] [--reps N] [--host-reps N] [--size WxH] [--label TEXT] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from videomorphing_amd import capi, morph, synth  # noqa: E402
from videomorphing_amd.viewport import Viewport  # noqa: E402

f32 = np.float32
FA = 0.5


def box2(img):
    """the host's half-size proxy: the mean of every 2 x 2 block of the rounded bytes, rounded again"""
    s = img.astype(np.float32)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]) * f32(0.25) + f32(0.5)).astype(np.uint8)


def bilinear(img, vp):
    """the host's zoom: a bilinear gather of the rounded bytes at the viewport's pixel centres, clamped to the frame"""
    h, w = img.shape[:2]
    x = (vp.x0 + (np.arange(vp.out_w, dtype=np.float32) + f32(0.5)) * f32(vp.step_x)) - f32(0.5)
    y = (vp.y0 + (np.arange(vp.out_h, dtype=np.float32) + f32(0.5)) * f32(vp.step_y)) - f32(0.5)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    a, b = (x - x0).astype(f32)[None, :, None], (y - y0).astype(f32)[:, None, None]
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    s = img.astype(np.float32)
    top = s[ya][:, xa] * (1 - a) + s[ya][:, xb] * a
    bot = s[yb][:, xa] * (1 - a) + s[yb][:, xb] * a
    return (top * (1 - b) + bot * b + f32(0.5)).astype(np.uint8)


def stat(x):
    return float(np.median(x)), float(np.min(x)), float(np.max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewport.md"))
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
    layers = {c: ((rng.rand(h, w, c).astype(f32)), (rng.rand(h, w, c).astype(f32))) for c in (1, 3, 4)}
    ident = Viewport.identity(w, h)
    proxy = Viewport.fit(w, h, w // 2, h // 2).supersampled(2)
    zoom = Viewport.zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 2.5, w // 4, h // 4)
    grids = (1, 2, 4)
    fr = morph.Frame(ctx, w, h, ex)
    dev_rows, host_rows = [], []
    for with_path in (False, True):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u if with_path else None)
        assert np.array_equal(fr.render_viewport(ident, FA, FA, 1), fr.render_halfway(FA, FA, 1))
        ts = {}
        for rep in range(a.reps + 2):                               # two rounds of warm-up
            got = {"u_rgb": fr.render_halfway_dev(FA, FA, 1)}
            for n in grids:
                got["v_rgb_%d" % n] = fr.render_viewport_dev(ident.supersampled(n), FA, FA, 1)
            got["proxy"] = fr.render_viewport_dev(proxy, FA, FA, 1)
            got["zoom"] = fr.render_viewport_dev(zoom, FA, FA, 1)
            for ch in (1, 3, 4):
                fr.upload_layers(*layers[ch])
                fr.render_layers_dev(FA, FA, 1)                     # (the first launch after an upload is not the timed one)
                got["u_l%d" % ch] = fr.render_layers_dev(FA, FA, 1)
                for n in grids:
                    got["v_l%d_%d" % (ch, n)] = fr.render_viewport_layers_dev(ident.supersampled(n), FA, FA, 1)
            if rep >= 2:
                for k, t in got.items():
                    ts.setdefault(k, []).append(t)
        dev_rows.append((with_path, {k: stat(x) for k, x in ts.items()}))
        # with the download, wall-clock, beside the host route
        wall = {k: [] for k in ("proxy", "proxy_host", "zoom", "zoom_host")}
        for _ in range(a.host_reps + 1):
            t0 = time.perf_counter(); p = fr.render_viewport(proxy, FA, FA, 1); t1 = time.perf_counter()
            ph = box2(fr.render_halfway(FA, FA, 1)); t2 = time.perf_counter()
            z = fr.render_viewport(zoom, FA, FA, 1); t3 = time.perf_counter()
            zh = bilinear(fr.render_halfway(FA, FA, 1), zoom); t4 = time.perf_counter()
            for k, t in zip(("proxy", "proxy_host", "zoom", "zoom_host"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                wall[k].append(1e3 * t)
        off_p = int(np.abs(p.astype(int) - ph.astype(int)).max())
        off_z = int(np.abs(z.astype(int) - zh.astype(int)).max())
        host_rows.append((with_path, {k: float(np.median(x[1:])) for k, x in wall.items()}, off_p, off_z))
    lines = [
        "%s The viewport calls at %dx%d beside what they replace: %s" % ("##" if a.append else "#", w, h, a.label),
        "",
        "Measured by `tools/dev_viewport.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the calls alternating" % (name.strip(), cus, a.reps),
        "within a round.  Field and path: those of `profiles/layer_warp.md`.  color_fa = geo_fa = %.1f, color_from 1.  Device events" % FA,
        "around each call, ms: median (minimum .. maximum over the rounds).  The numbers gate nothing.",
        "",
        "### 1, 2: the identity viewport with 1, 2 x 2 and 4 x 4 samples beside the uniform call",
        "",
        "| path | tail | uniform | viewport N = 1 | gap, us | N = 4 | / (4 x N = 1) | N = 16 | / (16 x N = 1) |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for with_path, ts in dev_rows:
        for tail, uk, vk in (("RGB8", "u_rgb", "v_rgb_%d"), ("1 ch", "u_l1", "v_l1_%d"), ("3 ch", "u_l3", "v_l3_%d"), ("4 ch", "u_l4", "v_l4_%d")):
            un, v1, v4, v16 = ts[uk], ts[vk % 1], ts[vk % 2], ts[vk % 4]
            lines.append("| %s | %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %+.1f | %.4f | %.2f | %.4f | %.2f |"
                         % (("yes" if with_path else "no", tail) + un + v1 + (1e3 * (v1[0] - un[0]), v4[0], v4[0] / (4 * v1[0]), v16[0], v16[0] / (16 * v1[0]))))
    lines += [
        "",
        "### 3, 4: a %dx%d proxy of 2 x 2 samples (steps 2: the plain form) and a %dx%d window of a 2.5x zoom" % (proxy.out_w, proxy.out_h, zoom.out_w, zoom.out_h),
        "",
        "Device ms as above; with the download, wall-clock ms, median of %d, beside `vm_render_halfway`, its download and the" % a.host_reps,
        "resample in numpy (a 2 x 2 box mean of the bytes; a bilinear gather of the bytes); `off`: the largest difference of the two",
        "pictures in grey levels (the host route resamples bytes that were rounded already, and filters the picture instead of",
        "the morph).",
        "",
        "| path | proxy, device | proxy + download | host route | off | zoom, device | zoom + download | host route | off |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for (with_path, ts), (_, wall, off_p, off_z) in zip(dev_rows, host_rows):
        lines.append("| %s | %.4f (%.4f .. %.4f) | %.2f | %.2f | %d | %.4f (%.4f .. %.4f) | %.2f | %.2f | %d |"
                     % (("yes" if with_path else "no",) + ts["proxy"] + (wall["proxy"], wall["proxy_host"], off_p) + ts["zoom"]
                        + (wall["zoom"], wall["zoom_host"], off_z)))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + "\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
