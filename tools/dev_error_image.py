"""Times the error view on a solved 1080p finest level against the route a host had before it existed, in one run:

  vm_level_energy                      vs  five vm_level_get_field downloads + the numpy statement + its sums
  vm_level_error_image to 1920x1080    vs  the same downloads + numpy planes + numpy sampling and ramp
  vm_level_energy_batch for 8 pairs    vs  eight times the first host route

Wall-clock medians of whole calls (launch, kernel, read-back, the stream drained), so the device figures are upper
bounds of the kernels' own time.  Writes a markdown note (default: profiles/error_image.md).  Development tool: the
numbers gate nothing.

  python tools/dev_error_image.py [--out PATH] [--reps N] [--iters K]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import error_ref as R  # noqa: E402
from videomorphing_amd import capi, morph, synth  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X data sheet


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_image.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    w, h, npairs = 1920, 1080, 8
    ctx = morph.Context(0, capi.MATH_FAST)
    P = morph.Parameters()
    P.bcond = capi.BCOND_BORDER
    ctx.set_params(morph.KernParameters(P))
    L = ctx._L
    name, cus, _ = ctx.device_info()
    v0 = (0.8 * synth.displacement(w, h)).astype(np.float32)
    cons, ncons = morph._cons_array(synth.make_constraints(w, h, 8))
    pyrs = []
    for k in range(npairs):
        i0, i1 = synth.make_pair(w, h, frame=k)
        p = morph.Pyramid(ctx)
        p.build_levels([(w, h), (w // 2, h // 2)])
        p.upload_luma(1, i0, i1)
        p[1].v = v0
        capi.check(L.vm_init_level(p._h, 0, w, h, cons, ncons))
        pr = capi.Progress()
        capi.check(L.vm_optimize_level(p._h, 0, float(a.iters), None, 1, C.byref(pr)))
        pyrs.append(p)
    p0 = pyrs[0]
    out5 = (C.c_double * 5)()
    out40 = (C.c_double * (5 * npairs))()
    arr = (C.c_void_p * npairs)(*[p._h for p in pyrs])
    rgb = np.zeros((h, w, 3), np.uint8)
    inv_wh = np.float32(1.0) / np.float32(w * h)

    def host_planes(p):
        lv = p[1]
        return R.planes(lv.field("value"), lv.field("v"), lv.field("tps_b"), lv.field("ui_axy"), lv.field("ui_b"), inv_wh, P)

    def host_energy(p):
        return [float(x.sum(dtype=np.float64)) for x in host_planes(p)]

    gain = 1.0 / float(np.median(host_planes(p0)[capi.ERR_SSIM]))
    t = {
        "energy_dev": median_ms(lambda: capi.check(L.vm_level_energy(p0._h, 0, out5)), a.reps),
        "energy_host": median_ms(lambda: host_energy(p0), max(a.reps // 4, 3)),
        "image_dev": median_ms(lambda: capi.check(L.vm_level_error_image(p0._h, 0, capi.ERR_SSIM, gain, w, h, rgb.ctypes.data, 0)), a.reps),
        "image_host": median_ms(lambda: R.image(host_planes(p0)[capi.ERR_SSIM], w, h, gain), max(a.reps // 4, 3)),
        "batch_dev": median_ms(lambda: capi.check(L.vm_level_energy_batch(arr, npairs, 0, out40)), a.reps),
        "batch_host": median_ms(lambda: [host_energy(p) for p in pyrs], 3),
    }
    # sanity of what was timed: the image is the statement's, the batch repeats the single call
    assert np.array_equal(rgb, R.image(host_planes(p0)[capi.ERR_SSIM], w, h, gain))
    capi.check(L.vm_level_energy(p0._h, 0, out5))
    assert list(out40[:5]) == list(out5)
    px = w * h
    e_bytes, i_bytes = 32 * px, 35 * px
    frac = lambda nbytes, ms: 100.0 * nbytes / (ms * 1e-3) / HBM_PEAK
    lines = [
        "# Error view at 1080p: the library's calls against the host route",
        "",
        "Measured by `tools/dev_error_image.py` on %s (%d CUs), FAST arithmetic, a 1920x1080 finest level after %d sweeps," % (name, cus, a.iters),
        "8 point pairs.  Medians of %d whole calls each (wall clock: launch, kernel, read-back, stream drained); the host" % a.reps,
        "route is what a caller had before: `vm_level_get_field` of value, v, tps_b, ui_axy and ui_b (32 B per pixel over the",
        "link) and the numpy statement of DESIGN.md 3.8 (`tests/error_ref.py`).  The numbers gate nothing.",
        "",
        "| call | library, ms | host route, ms | ratio |",
        "|---|---|---|---|",
        "| `vm_level_energy` | %.3f | %.1f | %.0fx |" % (t["energy_dev"], t["energy_host"], t["energy_host"] / t["energy_dev"]),
        "| `vm_level_error_image` to 1920x1080 | %.3f | %.1f | %.0fx |" % (t["image_dev"], t["image_host"], t["image_host"] / t["image_dev"]),
        "| `vm_level_energy_batch`, 8 pairs | %.3f | %.1f | %.0fx |" % (t["batch_dev"], t["batch_host"], t["batch_host"] / t["batch_dev"]),
        "",
        "Algorithmic bytes: `k_error_terms` reads 32 B per pixel (value, v, tps_b, ui_axy, ui_b; 44 B with the temporal term)",
        "= %.1f MB per 1080p level and writes %d partials of 40 B; `k_error_image` at ratio 1 reads the same and writes 3 B per" % (e_bytes / 1e6, ((w + 63) // 64) * ((h + 3) // 4)),
        "pixel = %.1f MB.  Against the %.0f TB/s HBM peak, counting the WHOLE call as if it were the kernel:" % (i_bytes / 1e6, HBM_PEAK / 1e12),
        "",
        "| call | bytes | %% of HBM peak (whole call) |",
        "|---|---|---|",
        "| `vm_level_energy` | %.1f MB | %.1f |" % (e_bytes / 1e6, frac(e_bytes, t["energy_dev"])),
        "| `vm_level_energy_batch`, 8 pairs | %.1f MB | %.1f |" % (npairs * e_bytes / 1e6, frac(npairs * e_bytes, t["batch_dev"])),
        "| `vm_level_error_image` (includes the 6.2 MB image crossing the link) | %.1f MB | %.1f |" % (i_bytes / 1e6, frac(i_bytes, t["image_dev"])),
        "",
        "The single calls are launch- and latency-bound, as expected of one pass over 66 MB; the batch shows what the pass",
        "itself reaches once eight levels share the launch.",
        "",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
