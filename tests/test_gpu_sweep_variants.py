"""Every FAST sweep kernel exists twice: the general one reads from the level's view whether its pages carry the
temporal term, the other is compiled without the term and is what the solver launches for levels that carry none
(profiles/sweep_variants.md).  vm_dbg_sweep_variant(ctx, 1) keeps the general kernels.

1  Specialised against general, bit for bit.  Each case runs twice on one context, under vm_dbg_sweep_variant 0 and 1:
   SHA-256 of v, the iterations and the activity counters are equal, and the forced schedule ran its own kernels.
   The cases are those of tests/line_search_cases.py (PASS / STEP / SPLIT at 120x68 and 75x26; SPARSE / TILE / listed
   TILE at the sizes that prune), the constrained family of tests/line_search_ladder_cases.py, and one whole vm_solve
   under the AUTO schedule.
2  The graph cache.  A cached hipGraph of TILE iterations holds fixed kernel nodes, so the variant belongs to its key
   (vm_sweep_sched.cpp: sweep_graph).  vm_video_optimize_level sweeps the middle page (no term) and then a tied page
   (with the term) through the SAME context, page count, geometry, buffers and parameters: without the variant in the
   key the tied page replays the graph captured for the middle page, with kernels that hold nothing of the term.  One
   context sweeps a plain 75x26 level, the two tied pages of line_search_ladder_cases._temporal_level, and the plain
   level again, forced TILE, 40 iterations a call (graph replays from the third iteration on); every result equals
   the same call on a fresh context, and the tied pages also equal a fresh context that keeps the general kernels --
   the comparison that fails when the variant is left out of the key, because a fresh context then makes the same
   mistake within the one video call."""
import ctypes as C

import numpy as np
import pytest

import line_search_cases as LC
import line_search_ladder_cases as LL
from videomorphing_amd import capi, morph, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fast_ctx(gpu_ctx):
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    yield gpu_ctx
    gpu_ctx.set_sweep_variant(0)
    gpu_ctx.set_math_mode(capi.MATH_EXACT)


def _both(ctx, run):
    """run() under the variant chosen by the level, then under the general kernels"""
    out = []
    try:
        for mode in (0, 1):
            ctx.set_sweep_variant(mode)
            out.append(run())
    finally:
        ctx.set_sweep_variant(0)
    return out


# ---- 1: specialised against general ------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,name,sched,parts", LC.cases())
def test_specialised_sweeps_equal_general_ones(fast_ctx, w, h, name, sched, parts):
    spec, gen = _both(fast_ctx, lambda: LC.run_case(fast_ctx, w, h, name, sched, parts))
    print(LC.key(w, h, name), spec["v_sha256"][:16], spec["totals"], spec["sched_launches"])
    for got in (spec, gen):
        assert got["sched_launches"][LC.SLOT[name]] > 0      # the kernels the case is about ran
        assert got["totals"][2] > 0                          # and moved pixels
    assert spec == gen


@pytest.mark.parametrize("name,sched,parts", LL.SCHEDULES)
def test_specialised_constrained_sweeps_equal_general_ones(fast_ctx, name, sched, parts):
    spec, gen = _both(fast_ctx, lambda: LL.run_case(fast_ctx, "constrained", name, sched, parts))
    print(LL.key("constrained", name), spec["v_sha256"][:16], spec["totals"], spec["sched_launches"])
    for got in (spec, gen):
        assert got["sched_launches"][LC.SLOT[name]] > 0
        assert got["totals"][0][2] > 0
    assert spec == gen


def test_specialised_solve_equals_general_one(fast_ctx):
    """a whole coarse-to-fine solve under the AUTO schedule, 150x100 from start_res 32"""
    w, h = 150, 100
    i0, i1 = synth.make_pair(w, h)
    prm = morph.Parameters()
    prm.max_iter, prm.max_iter_drop_factor, prm.start_res = 60, 1.0, 32
    kept = capi.KernParams()
    capi.check(fast_ctx._L.vm_get_params(fast_ctx._h, C.byref(kept)))

    def solve():
        fast_ctx.set_params(morph.KernParameters(prm))
        fast_ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        pyr = morph.Pyramid(fast_ctx)
        pyr.build(i0, i1, prm.start_res)
        nl = pyr.size() - 2
        prog = (capi.Progress * nl)()
        capi.check(pyr._L.vm_solve(pyr._h, float(prm.max_iter), 1.0, None, 0, None, 0, prog))
        return dict(v=LC._sha(pyr[1].v), iters=[int(prog[k].iters) for k in range(nl)],
                    counters=[[int(getattr(prog[k], c)) for c in LC.COUNTERS] for k in range(nl)],
                    launches=[[int(x) for x in prog[k].sched_launches] for k in range(nl)])

    try:
        spec, gen = _both(fast_ctx, solve)
    finally:
        fast_ctx.set_params(kept)
    print("solve %dx%d" % (w, h), spec["v"][:16], spec["iters"], spec["launches"])
    assert len(spec["iters"]) >= 2 and sum(c[2] for c in spec["counters"]) > 0
    assert spec == gen


# ---- 2: the graph key --------------------------------------------------------------------------------------------------

GW, GH = LL.W, LL.H                                       # 75x26
GSWEEPS = LC.SWEEPS                                       # batches of 2, 8 and 30 iterations: graph replays from the second on


def _plain(ctx):
    ctx.set_params(morph.KernParameters(morph.Parameters()))
    ctx.set_tuning(capi.SWEEP_TILE, 0, 0)
    pyr = LC._level(ctx, GW, GH, "tile_forced_dense")     # (not a PRUNED name: the noisy pair, the +-3 px start field)
    pr = capi.Progress()
    capi.check(pyr._L.vm_optimize_level(pyr._h, 0, float(GSWEEPS), None, 1, C.byref(pr)))
    launches = [int(x) for x in pr.sched_launches]
    assert int(pr.iters) == GSWEEPS >= 8 and launches[0] + launches[1] > 0 and not any(launches[2:]), launches
    return dict(v=LC._sha(pyr[1].v), counters=[int(getattr(pr, c)) for c in LC.COUNTERS])


def _tied(ctx):
    ctx.set_params(LL._params(w_temp=LL.W_TEMP))
    ctx.set_tuning(capi.SWEEP_TILE, 0, 0)
    dev = LL._temporal_level(ctx)
    prog = LL._temporal_sweeps(dev, GSWEEPS)
    launches = [int(x) for x in prog[0].sched_launches]
    assert [int(p.iters) for p in prog] == [GSWEEPS, GSWEEPS] and launches[0] + launches[1] > 0 and not any(launches[2:]), launches
    assert max(float(dev.pages[0][t].field("temp_mask").max()) for t in range(2)) > 0      # the term was there
    return dict(v=[LC._sha(dev.pages[0][t].v) for t in range(2)], counters=LL._counters(prog))


def _fresh(step, variant=0):
    ctx = morph.Context(0, capi.MATH_FAST)
    try:
        ctx.set_sweep_variant(variant)
        return step(ctx)
    finally:
        ctx.close()


def test_graph_cache_keeps_the_variants_apart():
    one = morph.Context(0, capi.MATH_FAST)
    try:
        got = [step(one) for step in (_plain, _tied, _plain)]
    finally:
        one.close()
    print("graph key:", got[0]["v"][:16], [s[:16] for s in got[1]["v"]], got[2]["v"][:16])
    assert got[0] == got[2]                                          # the same call from the same start
    assert got[0] == _fresh(_plain)
    assert got[1] == _fresh(_tied)
    general = _fresh(_tied, variant=1)                               # general kernels in every graph: the key cannot matter
    assert got[1] == general
    assert got[0] == _fresh(_plain, variant=1)
    assert got[1]["v"][0] != got[1]["v"][1]                          # two pages, two results
