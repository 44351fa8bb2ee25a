"""The 32-lane line search commits the lumas it committed while it carried the lumas of both candidate points through
every round of the golden section (profiles/line_search_carry.md): now it samples them once, at the accepted point of
the line, and only for a search that commits.

tests/golden/line_search_carry.json was recorded by tests/golden/make_line_search_carry.py with the library of the
PARENT commit of that change, never with the code under test: SHA-256 of v, luma, mean, var, cross, value and tps_b of
one level in FAST arithmetic, the four activity counters and the launches per schedule slot.  (The fixture of
tests/test_gpu_line_search_round.py hashes v alone; the lumas and the window sums made from them are what this change
could move.)  Without the temporal term: 120x68 and 75x26 with the inputs of tests/line_search_cases.py under forced
PASS and STEP, after 3 sweeps and after 40.  With it (w_temp = 25, two pages, one tied to the other as in
tests/test_gpu_temporal.py, both pages hashed): 90x50 and 75x26 under forced PASS, STEP and SPLIT, 40 sweeps, and the
level that prunes, 210x118, under forced SPARSE and TILE, 60 sweeps.  Every case asserts that its schedule's own
kernels ran and committed, the temporal ones that a page had a temporal mask.  Cases: tests/line_search_carry_cases.py."""
import json
import os

import pytest

import line_search_carry_cases as CC
from videomorphing_amd import capi

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_search_carry.json")))


@pytest.fixture(scope="module")
def fast_ctx(gpu_ctx):
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    yield gpu_ctx
    gpu_ctx.set_math_mode(capi.MATH_EXACT)


def test_fixture_covers_the_cases():
    assert "parent commit 31120a9" in GOLDEN["library"] and GOLDEN["arithmetic"] == "FAST"
    assert GOLDEN["fields"] == list(CC.FIELDS) and GOLDEN["counters"] == list(CC.COUNTERS) and GOLDEN["w_temp"] == CC.W_TEMP
    assert sorted(GOLDEN["cases"]) == sorted(c[0] for c in CC.cases())
    for key, kind, w, h, name, sweeps in CC.cases():
        c = GOLDEN["cases"][key]
        # the forced schedule ran its own kernels when the fixture was made and moved pixels, on every page all sweeps
        assert c["reached"] and CC.reached(name, c), key
        assert len(c["pages"]) == (2 if kind == "temporal" else 1), key
        assert all(p["iters"] == sweeps and sorted(p["sha256"]) == sorted(CC.FIELDS) for p in c["pages"]), key
        assert (c["temp_mask_max"] > 0) == (kind == "temporal"), key


@pytest.mark.gpu
@pytest.mark.parametrize("key,kind,w,h,name,sweeps", CC.cases(), ids=[c[0] for c in CC.cases()])
def test_fields_reproduce_the_parent_bits(fast_ctx, key, kind, w, h, name, sweeps):
    want = GOLDEN["cases"][key]
    got = CC.run_case(fast_ctx, kind, w, h, name, sweeps)
    print(key, [(p["sha256"]["luma"][:12], p["counters"], p["sched_launches"]) for p in got["pages"]], got["temp_mask_max"])
    assert sum(p["sched_launches"][CC.SLOT[name]] for p in got["pages"]) > 0      # the kernels the case is about ran
    assert sum(p["counters"][CC.COUNTERS.index("commits")] for p in got["pages"]) > 0
    if kind == "temporal":
        assert got["temp_mask_max"] > 0
    assert len(got["pages"]) == len(want["pages"])
    for t, (g, w_) in enumerate(zip(got["pages"], want["pages"])):
        assert g["iters"] == w_["iters"], (key, t)
        assert g["counters"] == w_["counters"], (key, t)
        assert g["sched_launches"] == w_["sched_launches"], (key, t)
        for f in CC.FIELDS:
            assert g["sha256"][f] == w_["sha256"][f], (key, t, f)
    assert got["temp_mask_max"] == want["temp_mask_max"]
