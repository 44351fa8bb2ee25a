"""The 32-lane line search gives the bits it gave before a lane kept its last texel across the evaluations of a search
(profiles/line_search_round.md).

tests/golden/line_search_round.json was recorded by tests/golden/make_line_search_round.py with the library of the
PARENT commit of that change (a load per evaluation), never with the code under test: SHA-256 of v after 40 sweeps of
one level in FAST arithmetic and the activity counters of every sweep, per forced schedule.  PASS / STEP / SPLIT: 120x68
(the benchmark's PASS level) and 75x26 (every tile clipped, every pixel a border pixel), noisy images, a start field of
up to +-3 px everywhere.  SPARSE / TILE / TILE in its listed form: levels that prune (240x135 and 200x170, the same noisy
image on both sides, a zero field but for small patches thrown off by up to +-3 px), because only pruned sweeps run
k_sparse, the lean k_optimize and k_optimize_listed -- and each case asserts that its kernels did run.  (A call's first
batch of sweeps is always dense: on those levels the hash and the totals of the 40-sweep call are the lean kernels',
the per-sweep counters and the second hash, from 40 calls of one sweep, the dense kernel's.)  Cases:
tests/line_search_cases.py."""
import json
import os

import pytest

import line_search_cases as LC
from videomorphing_amd import capi

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_search_round.json")))
_got = {}


def _case(ctx, w, h, name, sched, parts):
    """each case is run once and shared"""
    if (w, h, name) not in _got:
        _got[(w, h, name)] = LC.run_case(ctx, w, h, name, sched, parts)
    return _got[(w, h, name)]


@pytest.fixture(scope="module")
def fast_ctx(gpu_ctx):
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    yield gpu_ctx
    gpu_ctx.set_math_mode(capi.MATH_EXACT)


def test_fixture_covers_the_cases():
    assert GOLDEN["sweeps"] == LC.SWEEPS and GOLDEN["counters"] == list(LC.COUNTERS) and "parent commit" in GOLDEN["library"]
    assert sorted(GOLDEN["cases"]) == sorted(LC.key(w, h, n) for w, h, n, _, _ in LC.cases())
    # every forced schedule ran its own kernels when the fixtures were made, moved pixels, and kept searching to the end
    for k, c in GOLDEN["cases"].items():
        per = GOLDEN["per_sweep_tables"][c["per_sweep_table"]]
        assert c["reached"], k
        assert c["iters"] == LC.SWEEPS and c["totals"][2] > 0 and len(per) == LC.SWEEPS and per[-1][1] > 0, k


@pytest.mark.parametrize("w,h,name,sched,parts", LC.cases())
def test_schedule_reproduces_the_parent_bits(fast_ctx, w, h, name, sched, parts):
    want = GOLDEN["cases"][LC.key(w, h, name)]
    got = _case(fast_ctx, w, h, name, sched, parts)
    print(LC.key(w, h, name), got["v_sha256"][:16], got["totals"], got["sched_launches"])
    assert got["sched_launches"][LC.SLOT[name]] > 0          # the kernels the case is about ran
    assert got["iters"] == want["iters"]
    assert got["per_sweep"] == GOLDEN["per_sweep_tables"][want["per_sweep_table"]]
    assert got["totals"] == want["totals"]
    assert got["v_sha256"] == want["v_sha256"]
    assert got["v_sha256_single_sweeps"] == want["v_sha256_single_sweeps"]


@pytest.mark.parametrize("group,sizes", [(("pass", "step", "split"), LC.SIZES), (LC.PRUNED, LC.PRUNED_SIZES)])
def test_schedules_still_equal_each_other(fast_ctx, group, sizes):
    """the schedules agreed bit for bit in the parent and agree now: STEP == SPLIT == PASS, and SPARSE == TILE == listed
    TILE on the levels that prune"""
    sched = {n: (s, p) for n, s, p in LC.SCHEDULES}
    for w, h in sizes:
        got = {n: _case(fast_ctx, w, h, n, *sched[n])["v_sha256"] for n in group}
        gold = {n: GOLDEN["cases"][LC.key(w, h, n)]["v_sha256"] for n in group}
        assert len(set(gold.values())) == 1 and len(set(got.values())) == 1, (w, h, gold, got)
