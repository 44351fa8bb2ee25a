"""The cases of tests/test_gpu_line_search_carry.py and of the script that recorded its fixtures
(tests/golden/make_line_search_carry.py): one level in FAST arithmetic under a forced schedule, every field a commit of
the 32-lane line search writes -- the committed lumas and the window sums made from them, not v alone -- with and
without the temporal term.  No test here."""
import ctypes as C
import hashlib

import numpy as np

import line_search_cases as LC
from videomorphing_amd import capi, morph, synth

FIELDS = ("v", "luma", "mean", "var", "cross", "value", "tps_b")
COUNTERS = LC.COUNTERS
# [0] TILE dense, [1] TILE lean, [2] STEP / SPLIT, [3] SPARSE, [4] PASS (Progress.sched_launches)
SLOT = {"pass": 4, "step": 2, "split": 2, "sparse": 3, "tile": 1}
SCHED = {"pass": capi.SWEEP_PASS, "step": capi.SWEEP_STEP, "split": capi.SWEEP_SPLIT, "sparse": capi.SWEEP_SPARSE,
         "tile": capi.SWEEP_TILE}
W_TEMP = 25.0
PRUNED_SIZE = (210, 118)


def cases():
    """(key, kind, w, h, schedule name, sweeps).  plain: line_search_cases.inputs, hashed after 3 sweeps and after 40.
    temporal: two pages, one tied to the other (w_temp = 25), both hashed; 210x118 is the level that prunes"""
    out = []
    for w, h in LC.SIZES:
        for name in ("pass", "step"):
            for sweeps in (3, 40):
                out.append(("plain/%dx%d/%s/%d" % (w, h, name, sweeps), "plain", w, h, name, sweeps))
    for w, h in ((90, 50), (75, 26)):
        for name in ("pass", "step", "split"):
            out.append(("temporal/%dx%d/%s/40" % (w, h, name), "temporal", w, h, name, 40))
    for name in ("sparse", "tile"):
        out.append(("temporal/%dx%d/%s/60" % (PRUNED_SIZE + (name,)), "temporal") + PRUNED_SIZE + (name, 60))
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _progress(pr):
    return {"iters": int(pr.iters), "counters": [int(getattr(pr, k)) for k in COUNTERS],
            "sched_launches": [int(x) for x in pr.sched_launches]}


def _run_plain(ctx, w, h, name, sweeps):
    ctx.set_params(morph.KernParameters(morph.Parameters()))
    ctx.set_tuning(SCHED[name], 0, 0)
    i0, i1, v0 = LC.inputs(w, h)
    pyr = morph.Pyramid(ctx)
    pyr.build_levels([(w, h), (max((w + 1) // 2, 5), max((h + 1) // 2, 5))])
    pyr.upload_luma(1, i0, i1)
    pyr[1].v = v0
    capi.check(pyr._L.vm_init_level(pyr._h, 0, w, h, None, 0))
    pr = capi.Progress()
    capi.check(pyr._L.vm_optimize_level(pyr._h, 0, float(sweeps), None, 1, C.byref(pr)))
    return {"pages": [dict(_progress(pr), sha256={f: _sha(pyr[1].field(f)) for f in FIELDS})], "temp_mask_max": 0.0}


def _smooth_flow(rng, w, h, amp):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a, b, c, d = rng.rand(4) * 2 * np.pi
    fx = amp * np.sin(2 * np.pi * x / w + a) * np.cos(2 * np.pi * y / h + b) + 0.3 * amp
    fy = amp * np.cos(2 * np.pi * x / w + c) * np.sin(2 * np.pi * y / h + d) - 0.2 * amp
    return np.stack([fx, fy], -1).astype(np.float32)


def _pruned_video(ctx, w, h):
    """two pages that prune: the lean kernels take a sweep only while it searches fewer than a tenth of the pixels
    (line_search_cases.pruned_inputs).  Every page shows the same noisy image on both sides, both videos move along the
    same smooth flow, the start field is zero but for the patches of line_search_cases.patches, thrown off by up to
    +-3 px, differently on the two pages: a fixed point nearly everywhere, and around the patches the tied page is
    drawn towards what the other page made of its own"""
    levels = [(w, h, 2), ((w + 1) // 2, (h + 1) // 2, 2)]
    dev = morph.VideoPyramid(ctx)
    dev.build_levels(levels)
    i0 = LC.inputs(w, h)[0]
    rng = np.random.RandomState(11)
    fwd, bwd = _smooth_flow(rng, w, h, 1.2), _smooth_flow(rng, w, h, 1.2)
    rng = np.random.RandomState(7 * w + h)
    for t in range(2):
        dev.upload_luma(0, t, i0, i0.copy())
        dev.upload_flows(0, t, fwd, fwd.copy(), bwd, bwd.copy())
        v0 = np.zeros((h, w, 2), np.float32)
        for x0, y0, pw, ph in LC.patches(w, h):
            v0[y0:y0 + ph, x0:x0 + pw] = rng.uniform(-3.0, 3.0, (ph, pw, 2)).astype(np.float32)
        dev.pages[0][t].v = v0
    return dev


def _video(ctx, w, h):
    """two pages of noisy synthetic frames and four smooth flow fields per page (the device half of the video of
    tests/test_gpu_temporal.py), a start field of 0.7 of the true displacement plus noise"""
    if (w, h) == PRUNED_SIZE:
        return _pruned_video(ctx, w, h)
    levels = [(w, h, 2), ((w + 1) // 2, (h + 1) // 2, 2)]
    rng = np.random.RandomState(11)
    dev = morph.VideoPyramid(ctx)
    dev.build_levels(levels)
    frames = synth.page_frames(levels, dev.factor_t)
    base = [synth.make_pair(w, h, frame=t, amp=0.012 * w) for t in range(2)]
    base = [(a + 3.0 * rng.randn(h, w).astype(np.float32), b + 3.0 * rng.randn(h, w).astype(np.float32)) for a, b in base]
    pyrs = [synth.build_pyramid(a, b, 2) for a, b in base]
    fl = {k: [_smooth_flow(rng, w, h, 1.2) for _ in range(2)] for k in ("f0", "f1", "b0", "b1")}
    for t in range(2):
        i0, i1 = pyrs[frames[0][t]][0]
        dev.upload_luma(0, t, i0, i1)
        dev.upload_flows(0, t, fl["f0"][t], fl["f1"][t], fl["b0"][t], fl["b1"][t])
    rng = np.random.RandomState(17)
    for t in range(2):
        dev.pages[0][t].v = (0.7 * synth.displacement(w, h, amp=1.0) + 0.1 * rng.randn(h, w, 2)).astype(np.float32)
    return dev


def _run_temporal(ctx, w, h, name, sweeps):
    prm = morph.Parameters()
    prm.w_temp = W_TEMP
    ctx.set_params(morph.KernParameters(prm))
    ctx.set_tuning(SCHED[name], 0, 0)
    dev = _video(ctx, w, h)
    capi.check(dev._L.vm_video_init_level(dev._h, 0, None, 0))
    prog = (capi.Progress * 2)()
    capi.check(dev._L.vm_video_optimize_level(dev._h, 0, float(sweeps), None, 1, prog))
    pages = [dict(_progress(prog[t]), sha256={f: _sha(dev.pages[0][t].field(f)) for f in FIELDS}) for t in range(2)]
    return {"pages": pages, "temp_mask_max": float(max(dev.pages[0][t].field("temp_mask").max() for t in range(2)))}


def run_case(ctx, kind, w, h, name, sweeps):
    """-> {"pages": [per page: SHA-256 of every field of FIELDS, iters, the four counters, launches per schedule slot],
    "temp_mask_max"}.  The context must be in FAST arithmetic; its parameters and the forced schedule are put back."""
    kept = capi.KernParams()
    capi.check(ctx._L.vm_get_params(ctx._h, C.byref(kept)))
    try:
        return (_run_plain if kind == "plain" else _run_temporal)(ctx, w, h, name, sweeps)
    finally:
        ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        ctx.set_params(kept)


def reached(name, result):
    """the forced schedule's own kernels ran (on some page) and moved pixels"""
    return (sum(p["sched_launches"][SLOT[name]] for p in result["pages"]) > 0
            and sum(p["counters"][COUNTERS.index("commits")] for p in result["pages"]) > 0)
