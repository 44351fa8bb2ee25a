"""The sweep cases of tests/test_gpu_phase_chain.py and of the script that recorded their fixtures
(tests/golden/make_phase_chain.py): FAST arithmetic, 40 sweeps a case, every schedule forced.

  plain        tests/line_search_cases.py at 120x68 and 75x26 under PASS / STEP / SPLIT, at 240x135 under SPARSE / TILE
  temporal     the two tied pages of tests/line_search_ladder_cases.py (75x26): the general kernels
  edge         the shapes that put every branch of the start blocks' border-aware index selects to use, under PASS /
               STEP / SPLIT, with BCOND_BORDER and the six pulling constraints of the FAST audit: 69x21 (exactly one
               tile pitch), 70x22 (a one-pixel sliver tile in both directions), 64x16 (a tile with no gap), 66x18 (the
               image edge inside the +-2 reach of a tile); each cuts 5x5 mask blocks at its right and bottom edges
  solve        one vm_solve of 150x100 under AUTO

The protocol and the helpers are those of tests/line_search_cases.py.  No test here."""
import ctypes as C

import fast_audit_cases as fa
import line_search_cases as LC
import line_search_ladder_cases as LL
from videomorphing_amd import capi, morph, synth

SWEEPS = LC.SWEEPS
SCHEDULES3 = LL.SCHEDULES                                            # pass, step, split
PLAIN = [(w, h, n, s, p) for w, h, n, s, p in LC.cases()
         if (n in ("pass", "step", "split") and (w, h) in ((120, 68), (75, 26))) or (n in ("sparse", "tile") and (w, h) == (240, 135))]
EDGE_SIZES = [(69, 21), (70, 22), (64, 16), (66, 18)]
SOLVE = (150, 100)


def _edge_level(ctx, w, h):
    i0, i1, v0 = LC.inputs(w, h)
    cons = fa.constraints(fa._case(w, h, fa.BCOND_BORDER), v0)
    pyr = morph.Pyramid(ctx)
    pyr.build_levels([(w, h), ((w + 1) // 2, (h + 1) // 2)])
    pyr.upload_luma(1, i0, i1)
    pyr[1].v = v0
    ca, n = morph._cons_array(cons)
    capi.check(pyr._L.vm_init_level(pyr._h, 0, w, h, ca, n))
    return pyr


def run_edge(ctx, w, h, sched, parts):
    """-> dict as line_search_cases.run_case makes it.  The context must be in FAST arithmetic; its parameters and the
    forced schedule are put back."""
    out = {}
    kept = capi.KernParams()
    capi.check(ctx._L.vm_get_params(ctx._h, C.byref(kept)))
    try:
        ctx.set_params(LL._params(bcond=fa.BCOND_BORDER))
        ctx.set_tuning(sched, 0, parts)
        pyr = _edge_level(ctx, w, h)
        pr = capi.Progress()
        capi.check(pyr._L.vm_optimize_level(pyr._h, 0, float(SWEEPS), None, 1, C.byref(pr)))
        out["v_sha256"] = LC._sha(pyr[1].v)
        out["iters"] = int(pr.iters)
        out["totals"] = [int(getattr(pr, k)) for k in LC.COUNTERS]
        out["sched_launches"] = [int(x) for x in pr.sched_launches]
        pyr = _edge_level(ctx, w, h)
        per = []
        for _ in range(SWEEPS):
            pr = capi.Progress()
            capi.check(pyr._L.vm_optimize_level(pyr._h, 0, 1.0, None, 1, C.byref(pr)))
            per.append([int(getattr(pr, k)) for k in LC.COUNTERS])
        out["v_sha256_single_sweeps"] = LC._sha(pyr[1].v)
        out["per_sweep"] = per
    finally:
        ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        ctx.set_params(kept)
    return out


def run_solve(ctx):
    """a whole coarse-to-fine solve under the AUTO schedule, 150x100 from start_res 32 (as
    tests/test_gpu_sweep_variants.py runs it): SHA-256 of v, and per level the iterations, the counters, the launches"""
    w, h = SOLVE
    i0, i1 = synth.make_pair(w, h)
    prm = morph.Parameters()
    prm.max_iter, prm.max_iter_drop_factor, prm.start_res = 60, 1.0, 32
    kept = capi.KernParams()
    capi.check(ctx._L.vm_get_params(ctx._h, C.byref(kept)))
    try:
        ctx.set_params(morph.KernParameters(prm))
        ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        pyr = morph.Pyramid(ctx)
        pyr.build(i0, i1, prm.start_res)
        nl = pyr.size() - 2
        prog = (capi.Progress * nl)()
        capi.check(pyr._L.vm_solve(pyr._h, float(prm.max_iter), 1.0, None, 0, None, 0, prog))
        return dict(v_sha256=LC._sha(pyr[1].v), iters=[int(prog[k].iters) for k in range(nl)],
                    totals=[[int(getattr(prog[k], c)) for c in LC.COUNTERS] for k in range(nl)],
                    sched_launches=[[int(x) for x in prog[k].sched_launches] for k in range(nl)])
    finally:
        ctx.set_params(kept)


def cases():
    """(key, kind, slot name, args) of every case: kind picks the runner, args are its arguments after the context"""
    out = [("plain/" + LC.key(w, h, n), "plain", n, (w, h, n, s, p)) for w, h, n, s, p in PLAIN]
    out += [("temporal/" + LL.key("temporal", n), "temporal", n, ("temporal", n, s, p)) for n, s, p in SCHEDULES3]
    out += [("edge/%dx%d/%s" % (w, h, n), "edge", n, (w, h, s, p)) for w, h in EDGE_SIZES for n, s, p in SCHEDULES3]
    out += [("solve/%dx%d/auto" % SOLVE, "solve", None, ())]
    return out


def run(ctx, kind, args):
    return {"plain": LC.run_case, "temporal": LL.run_case, "edge": run_edge, "solve": run_solve}[kind](ctx, *args)


def families():
    """the groups of cases whose schedules must agree among themselves: {family: [key of PASS, of STEP, of SPLIT]}"""
    out = {}
    for k, kind, name, _ in cases():
        if name in ("pass", "step", "split"):
            out.setdefault(k.rsplit("/", 1)[0], []).append(k)
    return out
