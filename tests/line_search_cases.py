"""The cases of tests/test_gpu_line_search_round.py and of the script that recorded its fixtures
(tests/golden/make_line_search_round.py): one level, FAST arithmetic, 40 sweeps under every forced schedule that
reaches the 32-lane line search.  No test here."""
import ctypes as C
import hashlib

import numpy as np

from videomorphing_amd import capi, morph, synth

SWEEPS = 40
# 120x68: 8 tiles per pass, the PASS level of the 1080p benchmark.  75x26: 2x2 tiles, every tile clipped by the right /
# bottom edge and every pixel a border pixel (its 5x5 window or its taps leave the image): the border forms.
SIZES = [(120, 68), (75, 26)]
# ... and the sizes of the levels that prune (PRUNED schedules).  The lean kernels take a sweep only while it searches
# fewer than a tenth of the pixels; on the fixed point of pruned_inputs() the pixels along the image border stay
# candidates for good (~2 searches per sweep for each of the ~4 (w + h) of them), so a level prunes from about
# w h / (w + h) > 80 on (measured: 120x68, 75x26, 150x47 and 333x47 never left the dense kernel).
# 240x135: the benchmark's STEP level.  200x170: 3x9 tiles, the right column and the bottom row clipped, a patch in
# their corner.
PRUNED_SIZES = [(240, 135), (200, 170)]
# name, forced schedule, `parts` of vm_set_tuning (TILE: parts = 1 lowers the threshold of the listed form of a pruned
# pass to one workgroup -- k_tile_scan + k_optimize_listed instead of the lean k_optimize)
SCHEDULES = [("pass", capi.SWEEP_PASS, 0), ("step", capi.SWEEP_STEP, 0), ("split", capi.SWEEP_SPLIT, 0),
             ("sparse", capi.SWEEP_SPARSE, 0), ("tile", capi.SWEEP_TILE, 0), ("tile_listed", capi.SWEEP_TILE, 1)]
# the slot of Progress.sched_launches a forced schedule must have used for the case to say anything about it
# ([0] TILE dense, [1] TILE lean, [2] STEP / SPLIT, [3] SPARSE, [4] PASS)
SLOT = {"pass": 4, "step": 2, "split": 2, "sparse": 3, "tile": 1, "tile_listed": 1}
PRUNED = ("sparse", "tile", "tile_listed")
COUNTERS = ("improving", "candidates", "commits", "evaluations")


def inputs(w, h):
    """PASS / STEP / SPLIT: a noisy synthetic pair and a start field of up to +-3 px everywhere: taps cross texel
    boundaries and leave the image, every pixel stays a candidate for all the sweeps"""
    i0, i1 = synth.make_pair(w, h)
    rng = np.random.RandomState(1000 * w + h)
    i0 = np.clip(i0 + 6.0 * rng.randn(h, w), 0.0, 255.0).astype(np.float32)
    i1 = np.clip(i1 + 6.0 * rng.randn(h, w), 0.0, 255.0).astype(np.float32)
    v0 = rng.uniform(-3.0, 3.0, (h, w, 2)).astype(np.float32)
    return i0, i1, v0


def patches(w, h):
    """(x0, y0, width, height) of the patches of pruned_inputs(): in the interior, in the bottom right corner, across
    the gap between the tiles of a pass (x = 64..68, y = 16..20)"""
    return [(w // 3, h // 2, 5, 3), (w - 5, h - 2, 5, 2), (63, 15, 5, 2)]


def pruned_inputs(w, h):
    """TILE / SPARSE: their lean kernels (k_optimize<false>, k_optimize_listed, k_sparse: the 32-lane search) take over
    once a sweep searches fewer than a tenth of the pixels.  The same noisy image on both sides and a zero field is a
    fixed point -- the first, dense sweep finds no move and clears the mask -- except in a few small patches whose field
    is thrown off by up to +-3 px: the moves stay around them, and every later batch of sweeps is pruned."""
    i0, _, _ = inputs(w, h)
    rng = np.random.RandomState(7 * w + h)
    v0 = np.zeros((h, w, 2), np.float32)
    for x0, y0, pw, ph in patches(w, h):
        v0[y0:y0 + ph, x0:x0 + pw] = rng.uniform(-3.0, 3.0, (ph, pw, 2)).astype(np.float32)
    return i0, i0.copy(), v0


def _level(ctx, w, h, name):
    i0, i1, v0 = pruned_inputs(w, h) if name in PRUNED else inputs(w, h)
    pyr = morph.Pyramid(ctx)
    pyr.build_levels([(w, h), (max((w + 1) // 2, 5), max((h + 1) // 2, 5))])
    pyr.upload_luma(1, i0, i1)
    pyr[1].v = v0
    capi.check(pyr._L.vm_init_level(pyr._h, 0, w, h, None, 0))
    return pyr


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(ctx, w, h, name, sched, parts):
    """-> dict: SHA-256 of v after SWEEPS sweeps in ONE call (batched launches: what decides which kernels run) and
    after SWEEPS calls of one sweep, the counters of the one call, the counters of every sweep of the second run, the
    launches per schedule slot of the one call.  The context must be in FAST arithmetic; its parameters and the forced
    schedule are put back."""
    out = {}
    kept = capi.KernParams()
    capi.check(ctx._L.vm_get_params(ctx._h, C.byref(kept)))
    try:
        ctx.set_params(morph.KernParameters(morph.Parameters()))
        ctx.set_tuning(sched, 0, parts)
        pyr = _level(ctx, w, h, name)
        pr = capi.Progress()
        capi.check(pyr._L.vm_optimize_level(pyr._h, 0, float(SWEEPS), None, 1, C.byref(pr)))
        out["v_sha256"] = _sha(pyr[1].v)
        out["iters"] = int(pr.iters)
        out["totals"] = [int(getattr(pr, k)) for k in COUNTERS]
        out["sched_launches"] = [int(x) for x in pr.sched_launches]
        pyr = _level(ctx, w, h, name)
        per = []
        for _ in range(SWEEPS):
            pr = capi.Progress()
            capi.check(pyr._L.vm_optimize_level(pyr._h, 0, 1.0, None, 1, C.byref(pr)))
            per.append([int(getattr(pr, k)) for k in COUNTERS])
        out["v_sha256_single_sweeps"] = _sha(pyr[1].v)
        out["per_sweep"] = per
    finally:
        ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        ctx.set_params(kept)
    return out


def cases():
    """(w, h, name, schedule, parts) of every case"""
    return [(w, h, n, s, p) for n, s, p in SCHEDULES for w, h in (PRUNED_SIZES if n in PRUNED else SIZES)]


def key(w, h, name):
    return "%dx%d/%s" % (w, h, name)
