"""The sweep cases of tests/test_gpu_line_search_ladder.py and of the script that recorded their fixtures
(tests/golden/make_line_search_ladder.py): 75x26 (2x2 tiles, every tile clipped, every pixel a border pixel), FAST
arithmetic, 40 sweeps under forced PASS / STEP / SPLIT -- once with the temporal term in every round's energy, once
with pulling point constraints and the locks of BCOND_BORDER.  The protocol and the helpers are those of
tests/line_search_cases.py.  No test here."""
import ctypes as C

import numpy as np

import fast_audit_cases as fa
import line_search_cases as LC
from videomorphing_amd import capi, morph, synth

W, H = 75, 26
SWEEPS = LC.SWEEPS
SCHEDULES = [(n, s, p) for n, s, p in LC.SCHEDULES if n in ("pass", "step", "split")]
FAMILIES = ("temporal", "constrained")
W_TEMP = 25.0                                     # as tests/test_gpu_temporal.py ties a page to its neighbour


def _params(**kw):
    P = morph.Parameters()
    for k, v in kw.items():
        setattr(P, k, v)
    return morph.KernParameters(P)


def _smooth_flow(rng, w, h, amp):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a, b, c, d = rng.rand(4) * 2 * np.pi
    fx = amp * np.sin(2 * np.pi * x / w + a) * np.cos(2 * np.pi * y / h + b) + 0.3 * amp
    fy = amp * np.cos(2 * np.pi * x / w + c) * np.sin(2 * np.pi * y / h + d) - 0.2 * amp
    return np.stack([fx, fy], -1).astype(np.float32)


def _temporal_level(ctx):
    """two pages tied to each other (tests/test_gpu_temporal.py's set-up on the device alone): per page the noisy pair
    and the +-3 px start field of line_search_cases.inputs, four smooth flow fields per page"""
    levels = [(W, H, 2), ((W + 1) // 2, (H + 1) // 2, 2)]
    dev = morph.VideoPyramid(ctx)
    dev.build_levels(levels)
    rng = np.random.RandomState(11)
    i0, i1, v0 = LC.inputs(W, H)
    for t in range(2):
        a = np.clip(i0 + 3.0 * rng.randn(H, W), 0.0, 255.0).astype(np.float32)
        b = np.clip(i1 + 3.0 * rng.randn(H, W), 0.0, 255.0).astype(np.float32)
        dev.upload_luma(0, t, a, b)
        dev.upload_flows(0, t, *[_smooth_flow(rng, W, H, 1.2) for _ in range(4)])
        dev.pages[0][t].v = (v0 + 0.1 * rng.randn(H, W, 2)).astype(np.float32)
    capi.check(dev._L.vm_video_init_level(dev._h, 0, None, 0))
    return dev


def _temporal_sweeps(dev, n):
    prog = (capi.Progress * 2)()
    capi.check(dev._L.vm_video_optimize_level(dev._h, 0, float(n), None, 1, prog))
    return prog


def _constrained_level(ctx):
    """the noisy pair and the +-3 px start field, the six pulling constraints of the FAST audit (fast_audit_cases:
    points(), PULL), BCOND_BORDER in the parameters"""
    i0, i1, v0 = LC.inputs(W, H)
    case = fa._case(W, H, fa.BCOND_BORDER)
    cons = fa.constraints(case, v0)
    pyr = morph.Pyramid(ctx)
    pyr.build_levels([(W, H), ((W + 1) // 2, (H + 1) // 2)])
    pyr.upload_luma(1, i0, i1)
    pyr[1].v = v0
    ca, n = morph._cons_array(cons)
    capi.check(pyr._L.vm_init_level(pyr._h, 0, W, H, ca, n))
    return pyr


def _constrained_sweeps(pyr, n):
    pr = capi.Progress()
    capi.check(pyr._L.vm_optimize_level(pyr._h, 0, float(n), None, 1, C.byref(pr)))
    return [pr]


def _counters(prog):
    return [[int(getattr(p, k)) for k in LC.COUNTERS] for p in prog]


def run_case(ctx, family, name, sched, parts):
    """-> dict as line_search_cases.run_case makes it, the counters per page (one page: the constrained family).  The
    context must be in FAST arithmetic; its parameters and the forced schedule are put back."""
    make, sweeps, v_of = {
        "temporal": (_temporal_level, _temporal_sweeps, lambda d: np.stack([d.pages[0][t].v for t in range(2)])),
        "constrained": (_constrained_level, _constrained_sweeps, lambda p: p[1].v),
    }[family]
    out = {}
    kept = capi.KernParams()
    capi.check(ctx._L.vm_get_params(ctx._h, C.byref(kept)))
    try:
        ctx.set_params(_params(w_temp=W_TEMP) if family == "temporal" else _params(bcond=fa.BCOND_BORDER))
        ctx.set_tuning(sched, 0, parts)
        lvl = make(ctx)
        prog = sweeps(lvl, SWEEPS)
        out["v_sha256"] = LC._sha(v_of(lvl))
        out["iters"] = [int(p.iters) for p in prog]
        out["totals"] = _counters(prog)
        out["sched_launches"] = [int(x) for x in prog[0].sched_launches]
        if family == "temporal":
            out["temp_mask_max"] = float(max(lvl.pages[0][t].field("temp_mask").max() for t in range(2)))
        lvl = make(ctx)
        per = []
        for _ in range(SWEEPS):
            per.append(_counters(sweeps(lvl, 1)))
        out["v_sha256_single_sweeps"] = LC._sha(v_of(lvl))
        out["per_sweep"] = per
    finally:
        ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        ctx.set_params(kept)
    return out


def cases():
    """(family, name, schedule, parts) of every case"""
    return [(f, n, s, p) for f in FAMILIES for n, s, p in SCHEDULES]


def key(family, name):
    return "%dx%d/%s/%s" % (W, H, family, name)
