"""Times the layers' Poisson extension and what it costs the layer render calls, at 1080p with ex = 192 (canvases of
2304 x 1464), for profiles/layer_extension.md:

  vm_frame_extend_layers, 1, 3 and 4 channels    the call's own elapsed_ms (device events around everything it enqueues:
                                                 canvas, type map, fill, and per channel group set-up, solve and paste)
  vm_poisson_extend_frames on the same frame     the yardstick: the same solver on the RGB canvases (elapsed_ms)
  vm_render_layers_dev, vm_render_shutter_layers_dev (4 samples), 1 and 4 channels
      on tight layers, this library beside another build of it (--other PATH: the parent commit's), alternating run by
      run, one fresh process per run (`--child`), each run the median of --reps launches after a warm-up;
      then on extended layers beside tight ones, in this library

The child processes bind the handful of entry points they call themselves, so that a library from before the extension
loads.  Writes a markdown note (default: profiles/layer_extension_timing.md).  Development tool: the numbers gate nothing.

  python tools/dev_layer_ext.py [--out PATH] [--other LIB] [--runs N] [--reps N] [--size WxH] [--ex N]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

f32 = np.float32
GEO, COL, SAMPLES = 0.35, 0.35, 4


def inputs(w, h, c):
    from videomorphing_amd import synth
    rng = np.random.RandomState(3)
    d = synth.displacement(w, h)
    v = (d + 0.05 * rng.randn(h, w, 2)).astype(f32)                 # a solved field: smooth, rounding-rough
    return v, rng.rand(h, w, c).astype(f32), rng.rand(h, w, c).astype(f32)


def child(lib_path, w, h, ex, reps, extended):
    """one run in this process, on the library at lib_path: {"layers1": ms, "layers4": ms, "shutter1": ms, "shutter4": ms}"""
    L = C.CDLL(lib_path)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.vm_ctx_create.argtypes = [i, C.POINTER(vp)]
    L.vm_frame_create.argtypes = [vp, i, i, i, C.POINTER(vp)]
    L.vm_frame_upload.argtypes = [vp, vp, vp, vp, vp]
    L.vm_frame_upload_layers.argtypes = [vp, i, vp, vp, i]
    L.vm_render_layers_dev.argtypes = [vp, f, f, i, C.POINTER(f)]
    L.vm_render_shutter_layers_dev.argtypes = [vp, f, f, f, i, i, C.POINTER(f)]
    L.vm_last_error.restype = C.c_char_p

    def ok(rc):
        assert rc == 0, L.vm_last_error()

    ctx, fr = vp(), vp()
    ok(L.vm_ctx_create(0, C.byref(ctx)))
    ok(L.vm_frame_create(ctx, w, h, ex, C.byref(fr)))
    out, ms = {}, f(0)
    for c in (1, 4):
        v, l0, l1 = inputs(w, h, c)
        ok(L.vm_frame_upload(fr, None, None, v.ctypes.data, None))
        ok(L.vm_frame_upload_layers(fr, c, l0.ctypes.data, l1.ctypes.data, 0))
        if extended:
            L.vm_frame_extend_layers.argtypes = [vp, f, i, C.POINTER(i), C.POINTER(f), C.POINTER(f)]
            ok(L.vm_frame_extend_layers(fr, 1e-5, 20000, None, None, None))
        calls = {"layers%d" % c: lambda: L.vm_render_layers_dev(fr, COL, GEO, 1, C.byref(ms)),
                 "shutter%d" % c: lambda: L.vm_render_shutter_layers_dev(fr, COL, 0.2, 0.5, SAMPLES, 1, C.byref(ms))}
        for name, call in calls.items():
            t = []
            for rep in range(reps + 3):                             # three launches of warm-up
                ok(call())
                if rep >= 3:
                    t.append(ms.value)
            out[name] = float(np.median(t))
    print("CHILD " + json.dumps(out))


def run_child(lib_path, a, extended):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_path, "--size", a.size, "--ex", str(a.ex), "--reps", str(a.reps)]
    r = subprocess.run(cmd + (["--extended"] if extended else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("CHILD ")][0][6:])


def spread(runs, key):
    x = [r[key] for r in runs]
    return float(np.median(x)), float(np.min(x)), float(np.max(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_extension_timing.md"))
    ap.add_argument("--other", default=None, help="another build of the library (the parent commit's) to alternate with")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--ex", type=int, default=192)
    ap.add_argument("--child", default=None)
    ap.add_argument("--extended", action="store_true")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    if a.child:
        return child(a.child, w, h, a.ex, a.reps, a.extended)

    from videomorphing_amd import capi, morph, synth
    ctx = morph.Context(0)
    name, cus, _ = ctx.device_info()
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    fr = morph.Frame(ctx, w, h, a.ex)
    ext_rows = []
    rgb_ms, rgb_it = [], None
    for rep in range(4):                                            # one round of warm-up
        fr.upload_rgb(rgb0, rgb1)
        fr.upload(v=inputs(w, h, 1)[0])
        s1, s2, ms = fr.poisson_extend_both(1e-5)
        rgb_it = (s1[0], s2[0])
        if rep:
            rgb_ms.append(ms)
    for c in (1, 3, 4):
        v, l0, l1 = inputs(w, h, c)
        fr.upload_layers(l0, l1)
        t, its = [], None
        for rep in range(4):
            res, ms = fr.extend_layers(1e-5)
            its = [(g[0][0], g[1][0]) for g in res]
            if rep:
                t.append(ms)
        ext_rows.append((c, float(np.median(t)), float(np.min(t)), its))
    fr.upload_layers(rgb0.astype(f32), rgb1.astype(f32))            # the plate itself as a layer: the same right-hand side
    t = []
    for rep in range(4):
        res, ms = fr.extend_layers(1e-5)
        if rep:
            t.append(ms)
    plate = (float(np.median(t)), [(g[0][0], g[1][0]) for g in res])
    fr.close()
    ctx.close()

    mine = capi.LIB_PATH
    tight = {"this": [], "other": []}
    for _ in range(a.runs):                                         # alternating, run by run
        if a.other:
            tight["other"].append(run_child(a.other, a, False))
        tight["this"].append(run_child(mine, a, False))
    extended = [run_child(mine, a, True) for _ in range(a.runs)]

    keys = ("layers1", "layers4", "shutter1", "shutter4")
    lines = [
        "## Timing at %dx%d, ex = %d (canvases of %dx%d)" % (w, h, a.ex, w + 2 * a.ex, h + 2 * a.ex),
        "",
        "Measured by `tools/dev_layer_ext.py` on %s (%d CUs).  The numbers gate nothing." % (name, cus),
        "",
        "### The extension beside the RGB extension of the same frame (tol 1e-5, elapsed_ms of the call, median of 3 after a warm-up)",
        "",
        "| call | ms | iterations (side 1, side 2) per group |",
        "|---|---|---|",
        "| `vm_poisson_extend_frames`, one frame | %.2f | %s |" % (float(np.median(rgb_ms)), rgb_it),
    ]
    for c, med, mn, its in ext_rows:
        lines.append("| `vm_frame_extend_layers`, %d channel%s of noise in [0, 1] | %.2f (min %.2f) | %s |" % (c, "" if c == 1 else "s", med, mn, its))
    lines.append("| `vm_frame_extend_layers`, the frame's RGB as a 3-channel layer | %.2f | %s |" % plate)
    lines += [
        "",
        "### The layer render calls on tight layers, this build beside the other one",
        "",
        "One fresh process per run, the two libraries alternating run by run, %d runs each; a run is the median of %d launches" % (a.runs, a.reps),
        "(device events) after three of warm-up.  geo_fa = color_fa = %.2f; the shutter takes %d samples over [0.2, 0.5].  Median" % (GEO, SAMPLES),
        "of the runs (smallest .. largest run).",
        "",
        "| call | other build, ms | this build, ms | this build, extended layers, ms |",
        "|---|---|---|---|",
    ]
    label = {"layers1": "`vm_render_layers_dev`, 1 channel", "layers4": "`vm_render_layers_dev`, 4 channels",
             "shutter1": "`vm_render_shutter_layers_dev`, 1 channel", "shutter4": "`vm_render_shutter_layers_dev`, 4 channels"}
    fmt = lambda s: "%.4f (%.4f .. %.4f)" % s
    for k in keys:
        lines.append("| %s | %s | %s | %s |" % (label[k], fmt(spread(tight["other"], k)) if a.other else "-", fmt(spread(tight["this"], k)),
                                              fmt(spread(extended, k))))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
