"""Three audits of VM_MATH_FAST -- the arithmetic every timed figure runs -- against the CPU oracle, under pulling point
constraints, the boundary conditions and ragged / sub-tile levels (cases: tests/fast_audit_cases.py).  Elsewhere FAST meets
constraints and border locks only next to FAST under another schedule; a mistake confined to the FAST instantiations (a
border-class thin-plate coefficient, an ignored lock, a ui term of energy_change, the ui_b update of a commit, a counter
in the border band) passes there.  No bound below comes from FAST's own output: each is a figure of the project cited in
fast_audit_cases, or a figure of the oracle computed here.

  1  one sweep from the same state, |dv| by pixel class, under every schedule
  2  the state FAST keeps incrementally equals its definition (a fresh init + splat from FAST's own v), at every pixel
  3  FAST's converged field is a fixed point of the reference
"""
import ctypes as C

import numpy as np
import pytest

import fast_audit_cases as fa
from videomorphing_amd import capi, morph

pytestmark = pytest.mark.gpu

_ids = lambda cases: [c.name for c in cases]
SCHEDULES = {"tile": capi.SWEEP_TILE, "split": capi.SWEEP_SPLIT, "step": capi.SWEEP_STEP, "pass": capi.SWEEP_PASS,
             "auto": capi.SWEEP_AUTO}


def _kp(P):
    k = capi.KernParams()
    for f, _ in capi.KernParams._fields_:
        setattr(k, f, getattr(P, f))
    return k


class _fast(object):
    """with _fast(gpu_ctx, sched): FAST arithmetic under one schedule; EXACT / AUTO again afterwards"""

    def __init__(self, ctx, sched, mode=capi.MATH_FAST):
        self.ctx, self.sched, self.mode = ctx, sched, mode

    def __enter__(self):
        self.ctx.set_math_mode(self.mode)
        self.ctx.set_tuning(self.sched, 0, 0)

    def __exit__(self, *a):
        self.ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        self.ctx.set_math_mode(capi.MATH_EXACT)


def _gpu_level(gpu_ctx, case):
    """the case's start on the device, initialised with the same constraints (as test_gpu_parity._make_level does)"""
    i0, i1, v0, cons = fa.start(case)
    w, h = case.w, case.h
    gpu_ctx.set_params(_kp(fa.params(case)))
    pyr = morph.Pyramid(gpu_ctx)
    pyr.build_levels([(w, h), (max((w + 1) // 2, 5), max((h + 1) // 2, 5))])
    pyr.upload_luma(1, i0, i1)
    pyr[1].v = v0
    ca, n = morph._cons_array(cons)
    capi.check(pyr._L.vm_init_level(pyr._h, 0, w, h, ca, n))
    return pyr


def _sweep(pyr, iters):
    pr = capi.Progress()
    capi.check(pyr._L.vm_optimize_level(pyr._h, 0, float(iters), None, 0, C.byref(pr)))
    return pr


# ---- Audit 1 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("case", fa.SWEEP_CASES, ids=_ids(fa.SWEEP_CASES))
def test_one_fast_sweep_matches_the_oracle_by_pixel_class(gpu_ctx, oracle, case, sched):
    """One FAST sweep and one oracle sweep from the same state.  Ring and rest: |dv| <= EPS on >= 99 % of the class and
    <= 2 EPS on all of it; footprint: every pixel <= 2 EPS (test_fast_mode_tolerance's bounds, per class).  The teeth
    (fast_audit_cases.check_sweep_conditions, the oracle alone): every free footprint pixel moves >= 0.5 px in this sweep,
    the outermost rows and columns do not move at all under BORDER, and the oracle's own four commit orders stay within EPS
    in every class -- so a dropped ui term, an ignored lock or a wrong border coefficient is not within the allowance."""
    fa.check_sweep_conditions(case)
    ref, masks, lock = fa.oracle_sweeps(case, 1, 0), fa.class_masks(case), fa.locked_mask(case)
    with _fast(gpu_ctx, SCHEDULES[sched]):
        pyr = _gpu_level(gpu_ctx, case)
        pr = _sweep(pyr, 1)
        v = pyr[1].v
    assert pr.iters == 1 and pr.commits > 0
    d = fa.pixel_diff(v, ref)
    fig = {c: (float((d[masks[c]] <= fa.EPS).mean()) if masks[c].any() else 1.0, m) for c, m in fa.class_max(d, masks).items()}
    print("audit1 %s %s (fraction within EPS, max px) %r" % (case.name, sched, fig))
    if lock.any():
        assert np.array_equal(v[lock].view(np.uint32), fa.start(case)[2][lock].view(np.uint32)), "a locked pixel moved"
    for c in fa.CLASSES:
        frac, worst = fig[c]
        assert worst <= 2 * fa.EPS, (case.name, sched, c, fig, np.argwhere((d > 2 * fa.EPS) & masks[c])[:8].tolist())
        if c != "footprint":
            assert frac >= 0.99, (case.name, sched, c, fig)


# ---- Audit 2 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", ["tile", "pass"])
@pytest.mark.parametrize("case", fa.STATE_CASES, ids=_ids(fa.STATE_CASES))
def test_fast_state_equals_its_definition_borders_and_constraints_included(gpu_ctx, oracle, case, sched):
    """After 1 and after 20 FAST sweeps: download v, build a fresh oracle level from it (init, splat with the same
    constraints) and compare every array the sweep maintains incrementally -- luma, mean, var, cross, value, tps_b, ui_b --
    at EVERY pixel, and the three it must not touch -- counter, tps_axy, ui_axy.  Tolerance per field: the oracle's own
    drift D_f over the same number of sweeps from the same start (its incremental arrays against a fresh init + splat of
    its own v) is the yardstick; FAST gets max(8 D_f, 4 float32 ulps of the field's magnitude).  A dropped or mis-weighted
    update is wrong by the step times a coefficient, three to five decades above that."""
    done = 0
    with _fast(gpu_ctx, SCHEDULES[sched]):
        pyr = _gpu_level(gpu_ctx, case)
        before = {f: pyr[1].field(f) for f in fa.UNTOUCHED}
        for n in fa.STATE_SWEEPS:
            fa.check_state_conditions(case, n)
            tol = fa.state_tolerance(case, n)
            _sweep(pyr, n - done)
            done = n
            state = {f: pyr[1].field(f) for f in fa.INCREMENTAL + fa.UNTOUCHED}
            err, mag, fresh = fa.state_error(state, case, pyr[1].v)
            D = fa.oracle_drift(case, n)[0]
            print("audit2 %s %s after %d: error / D_f %r" % (case.name, sched, n, {f: "%.3g / %.3g" % (err[f], D[f]) for f in fa.INCREMENTAL}))
            for f in fa.UNTOUCHED:
                assert np.array_equal(state[f].view(np.uint32), before[f].view(np.uint32)), (case.name, sched, n, f, "written to")
                ulp4 = 4 * float(np.spacing(np.float32(mag[f])))
                assert err[f] <= ulp4, (case.name, sched, n, f, err[f], ulp4)
            for f in fa.INCREMENTAL:
                bad = np.argwhere(np.abs(state[f].astype(np.float64) - fresh[f]).reshape(case.h, case.w, -1).max(-1) > tol[f])
                assert err[f] <= tol[f], (case.name, sched, n, f, err[f], tol[f], "pixels (y, x):", bad[:8].tolist())


# ---- Audit 3 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", fa.FIXED_POINT_CASES, ids=_ids(fa.FIXED_POINT_CASES))
def test_fast_converged_field_is_a_fixed_point_of_the_reference(gpu_ctx, oracle, case):
    """Comparing trajectories is statistical; this is not.  FAST runs to convergence (<= 2000 sweeps, asserted); its final v
    goes to a fresh oracle level (init, splat, full mask), which makes ONE sweep.  Yardstick, the reference alone: from its
    own fixed points under commit orders 0 - 2 such a sweep commits some hundred rounding-level moves, none above `figure`
    (0.0058 - 0.0079 px).  Asserted: from FAST's fixed point no pixel of any class moves more than max(EPS, 1.5 figure); FAST's
    field lies within 0.02 px RMS of the oracle's order-0 fixed point (the bound of
    test_fast_energy_on_converged_solves_sits_at_the_chaos_floor); the constraint total of the oracle's energy() of FAST's
    field is within max(0.5 %, 1.5 x the spread of the three oracle runs) of the order-0 run."""
    figure, spread, _ = fa.check_fixed_point_conditions(case)
    ref_v, _, _, _, ref_e = fa.oracle_fixed_point(case, 0)
    with _fast(gpu_ctx, capi.SWEEP_AUTO):
        pyr = _gpu_level(gpu_ctx, case)
        pr = _sweep(pyr, fa.FIXED_POINT_CAP)
        v = pyr[1].v
    assert pr.improving == 0 and pr.iters < fa.FIXED_POINT_CAP, (case.name, pr.iters, pr.improving)        # converged
    move, commits, energy = fa.fresh_sweep(case, v)
    rms = fa.rms_distance(v, ref_v)
    rel = abs(energy[2] - ref_e[2]) / ref_e[2]
    print("audit3 %s: %d sweeps; fresh oracle sweep: %d commits, moves %r (oracle figure %.4f); RMS to order 0 %.4f; "
          "constraint total %.4f vs %.4f (%.3f %%, oracle spread %.3f %%)"
          % (case.name, pr.iters, commits, move, figure, rms, energy[2], ref_e[2], 100 * rel, 100 * spread))
    lock = fa.locked_mask(case)
    if lock.any():
        assert np.array_equal(v[lock].view(np.uint32), fa.start(case)[2][lock].view(np.uint32)), "a locked pixel moved"
    cap = max(fa.EPS, 1.5 * figure)
    for c in fa.CLASSES:
        assert move[c] <= cap, (case.name, c, move, cap)
    assert rms <= 0.02, (case.name, rms)
    assert rel <= max(0.005, 1.5 * spread), (case.name, energy[2], ref_e[2], spread)
