"""The sweep driver's policy (videomorphing_amd/csrc/vm_sweep_plan.h: which schedule a batch of iterations runs, with
how many threads and parts, through which kernel form) is a header of pure functions that plain g++ compiles.  A small
driver prints the plans of a table of cases; the expected values are derived by hand from the rules DESIGN.md
section 3.1 states (tiles per pass: 60x34 -> 2, 120x68 -> 8, 240x135 -> 28, 480x270 -> 91, 960x540 -> 364,
1920x1080 -> 1456, 3840x2160 -> 5768)."""
import os
import subprocess

import pytest

from videomorphing_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videomorphing_amd", "csrc")

DRIVER = r"""
#include "vm_sweep_plan.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <iostream>
#include <sstream>

// one case per line: w h n math_mode sweep_mode threads parts latched test_timeout cand_prev tiles_prev may_pass [switch=value ...]
int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--env")) {
        const SweepSwitches &e = SweepSwitches::from_environment();
        printf("step_max_tiles=%d step_big_parts=%d corun_min_wgs=%d tile_list_min=%d pass_max_groups=%d sparse_tiles=%d "
               "step_min_cand=%g no_corun=%d no_tile_list=%d no_pass=%d tile_dense=%d dense128=%d\n",
               e.step_max_tiles, e.step_big_parts, e.corun_min_wgs, e.tile_list_min, e.pass_max_groups, e.sparse_tiles,
               e.step_min_cand, e.no_corun, e.no_tile_list, e.no_pass, e.tile_dense, e.dense128);
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--env-dense-noint")) {
        printf("%d\n", SweepSwitches::from_environment().dense_noint);
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        SweepCall q;
        SweepSwitches sw;
        int latched, tt, may_pass;
        double cand, tiles;
        in >> q.w >> q.h >> q.n >> q.math_mode >> q.sweep_mode >> q.sweep_threads >> q.sweep_parts >> latched >> tt >> cand >> tiles >> may_pass;
        q.pass_latched_off = latched != 0;
        q.pass_test_timeout = tt != 0;
        std::string kv;
        while (in >> kv) {
            const std::string k = kv.substr(0, kv.find('=')), v = kv.substr(kv.find('=') + 1);
            if (k == "step_max_tiles") sw.step_max_tiles = atoi(v.c_str());
            else if (k == "step_min_cand") sw.step_min_cand = atof(v.c_str());
            else if (k == "sparse_tiles") sw.sparse_tiles = atoi(v.c_str());
            else if (k == "no_corun") sw.no_corun = atoi(v.c_str()) != 0;
            else if (k == "no_tile_list") sw.no_tile_list = atoi(v.c_str()) != 0;
            else if (k == "no_pass") sw.no_pass = atoi(v.c_str()) != 0;
            else if (k == "tile_dense") sw.tile_dense = atoi(v.c_str()) != 0;
            else if (k == "dense128") sw.dense128 = atoi(v.c_str());
            else if (k == "dense_noint") sw.dense_noint = atoi(v.c_str());
            else return 2;
        }
        const SweepLevelPlan p = plan_level(q, sw);
        const SweepBatchPlan b = plan_batch(p, cand, tiles, may_pass != 0);
        printf("tiles=%d threads=%d parts=%d needs_ws=%d may_split=%d may_sparse=%d listed_ok=%d small_dense_ok=%d dense128=%d "
               "want_pass=%d pass_switches=%d forced_split=%d sched=%d dense=%d step=%d use_tile_list=%d small_dense=%d "
               "no_interior=%d tile_form=%d\n",
               p.tiles, p.threads, p.parts, p.needs_ws, p.may_split, p.may_sparse, p.listed_ok, p.small_dense_ok, p.dense128,
               p.want_pass, p.pass_switches, p.forced_split, (int)b.sched, b.dense, b.step, b.use_tile_list, b.small_dense,
               b.no_interior, b.tile_form());
    }
    return 0;
}
"""

FAST, EXACT = capi.MATH_FAST, capi.MATH_EXACT
AUTO, TILE, SPLIT, STEP, SPARSE, PASS = range(6)
FIRST = 1e9  # the counters "of the batch before the first": dense


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("sweep_plan")
    src = d / "plan.cpp"
    src.write_text(DRIVER)
    exe = str(d / "plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    return exe


def _plan(exe, w, h, n=1, math=FAST, mode=AUTO, threads=0, parts=0, latched=0, test_timeout=0, cand=FIRST, tiles=FIRST,
          token=False, **switches):
    line = "%d %d %d %d %d %d %d %d %d %r %r %d" % (w, h, n, math, mode, threads, parts, latched, test_timeout, float(cand), float(tiles), token)
    line += "".join(" %s=%s" % kv for kv in switches.items())
    out = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout.split()
    return {k: int(v) for k, v in (f.split("=") for f in out)}


def _has(got, **want):
    assert {k: got[k] for k in want} == want


def test_the_modes_and_schedules_are_numbered_as_the_abi_numbers_them():
    hdr = open(os.path.join(ROOT, "include", "vmorph.h")).read()
    assert "VM_SWEEP_AUTO = 0, VM_SWEEP_TILE = 1, VM_SWEEP_SPLIT = 2, VM_SWEEP_STEP = 3, VM_SWEEP_SPARSE = 4, VM_SWEEP_PASS = 5" in hdr
    assert (FAST, EXACT) == (1, 0)


@pytest.mark.parametrize("w,h,tiles", [(60, 34, 2), (120, 68, 8), (240, 135, 28), (480, 270, 91), (960, 540, 364),
                                       (1920, 1080, 1456), (3840, 2160, 5768)])
def test_tiles_per_pass(plan_exe, w, h, tiles):
    assert _plan(plan_exe, w, h)["tiles"] == tiles


def test_smallest_level_of_a_single_pair_runs_pass_with_the_token_and_step_without(plan_exe):
    _has(_plan(plan_exe, 120, 68, token=True), want_pass=1, sched=4, step=0, parts=32, needs_ws=1, may_split=1)
    _has(_plan(plan_exe, 120, 68, token=False), want_pass=1, sched=2, step=1, parts=32)


def test_batches_of_the_smallest_level(plan_exe):
    # 4 pairs: 32 tile groups > 8: no PASS; STEP with 16 parts
    _has(_plan(plan_exe, 120, 68, n=4), want_pass=0, sched=2, step=1, parts=16, may_split=1)
    # 8 pairs: 64 groups, the last batch size that may split: 8 parts
    _has(_plan(plan_exe, 120, 68, n=8), may_split=1, needs_ws=1, parts=8, sched=2, step=1)
    # 9 pairs: TILE, dense first (<= 32 tiles per pass: 256-thread workgroups may pair up)
    _has(_plan(plan_exe, 120, 68, n=9), may_split=0, needs_ws=0, sched=0, dense=1, small_dense_ok=1, small_dense=1, parts=8)


def test_auto_leaves_step_below_200_line_searches_per_iteration_and_pair(plan_exe):
    _has(_plan(plan_exe, 240, 135, cand=200), sched=2, step=1, parts=16, want_pass=0)
    _has(_plan(plan_exe, 240, 135, cand=199, tiles=12.5), sched=1, dense=0, step=0, small_dense=0)
    _has(_plan(plan_exe, 240, 135, cand=199, tiles=12), sched=3, dense=0)
    # per pair: two pairs split down to 400
    _has(_plan(plan_exe, 240, 135, n=2, cand=400), sched=2)
    _has(_plan(plan_exe, 240, 135, n=2, cand=399), sched=1)


def test_dense_kernel_form_goes_by_the_level_size(plan_exe):
    _has(_plan(plan_exe, 480, 270), sched=0, dense=1, dense128=0, small_dense_ok=0, small_dense=0, may_split=0, needs_ws=0)
    _has(_plan(plan_exe, 960, 540), sched=0, dense=2, dense128=1)
    # ... never by the batch: 30 pairs of 480x270 keep the 256-VGPR form
    _has(_plan(plan_exe, 480, 270, n=30), dense=1, dense128=0)


def test_small_levels_run_the_dense_kernel_without_its_interior_form(plan_exe):
    """FAST, a dense batch that is not the 128-VGPR form: the form without the interior body up to 32 tiles per pass
    (tile_form 3 is what the TILE launcher is told; `dense` stays 1)."""
    _has(_plan(plan_exe, 276, 168, mode=TILE), tiles=32, sched=0, dense=1, no_interior=1, tile_form=3)  # 4 x 8
    _has(_plan(plan_exe, 207, 231, mode=TILE), tiles=33, sched=0, dense=1, no_interior=0, tile_form=1)  # 3 x 11
    _has(_plan(plan_exe, 240, 135, mode=TILE), tiles=28, sched=0, dense=1, no_interior=1, tile_form=3)
    _has(_plan(plan_exe, 1920, 1080), sched=0, dense=2, no_interior=0, tile_form=2)
    _has(_plan(plan_exe, 1920, 1080, dense128=0), sched=0, dense=1, no_interior=0, tile_form=1)
    # a rule on the level, never on the batch: AUTO's TILE batches of many pairs, the dense ones of a pruned level
    _has(_plan(plan_exe, 276, 168, n=3), sched=0, dense=1, no_interior=1, tile_form=3)
    _has(_plan(plan_exe, 207, 231, n=30), sched=0, dense=1, no_interior=0, tile_form=1)
    _has(_plan(plan_exe, 240, 135, cand=10, tiles=100, tile_dense=1), sched=0, dense=1, no_interior=1, tile_form=3)


def test_the_no_interior_switch_and_what_it_never_touches(plan_exe):
    levels = [(120, 68), (276, 168), (207, 231), (240, 135), (480, 270), (960, 540), (1920, 1080)]
    # forced off: no level gets the form
    for w, h in levels:
        got = _plan(plan_exe, w, h, mode=TILE, dense_noint=0)
        _has(got, no_interior=0, tile_form=got["dense"])
    # forced on: every dense FAST batch that is not the 128-VGPR form gets it ...
    for w, h in levels:
        _has(_plan(plan_exe, w, h, mode=TILE, dense128=0, dense_noint=1), dense=1, no_interior=1, tile_form=3)
    # ... and a batch planned as the 128-VGPR form never does, by the level's size or forced
    for w, h in ((960, 540), (1920, 1080)):
        _has(_plan(plan_exe, w, h, mode=TILE, dense_noint=1), dense128=1, dense=2, no_interior=0, tile_form=2)
    _has(_plan(plan_exe, 120, 68, mode=TILE, dense128=1), dense=2, no_interior=0, tile_form=2)
    _has(_plan(plan_exe, 120, 68, mode=TILE, dense128=1, dense_noint=1), dense=2, no_interior=0, tile_form=2)
    # EXACT and the diagnostic arithmetics have one dense form
    for m in (EXACT, capi.MATH_EXACT_FMA, capi.MATH_REF_FASTMATH, capi.MATH_REF_TEX8, capi.MATH_REF_TEX8_TRUNC):
        _has(_plan(plan_exe, 240, 135, math=m, mode=TILE), dense=1, no_interior=0, tile_form=1)
        _has(_plan(plan_exe, 240, 135, math=m, mode=TILE, dense_noint=1), dense=1, no_interior=0, tile_form=1)
    # a lean batch is untouched
    _has(_plan(plan_exe, 240, 135, mode=TILE, cand=10, tiles=100), sched=1, dense=0, no_interior=0, tile_form=0)
    _has(_plan(plan_exe, 240, 135, mode=TILE, cand=10, tiles=100, dense_noint=1), sched=1, dense=0, no_interior=0, tile_form=0)
    _has(_plan(plan_exe, 240, 135, cand=10, tiles=1, dense_noint=1), sched=3, dense=0, no_interior=0, tile_form=0)


def test_the_no_interior_switch_comes_from_the_environment(plan_exe):
    def dense_noint(**env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("VM_")}
        e.update(env)
        return int(subprocess.run([plan_exe, "--env-dense-noint"], env=e, capture_output=True, text=True, check=True).stdout)
    assert dense_noint() == -1
    assert dense_noint(VM_DENSE_NOINT="0") == 0
    assert dense_noint(VM_DENSE_NOINT="1") == 1
    assert dense_noint(VM_DENSE_NOINT="7") == 1
    assert dense_noint(VM_DENSE_NOINT="x") == 0  # atoi


def test_lean_regime_starts_below_a_tenth_of_the_pixels(plan_exe):
    _has(_plan(plan_exe, 1920, 1080, cand=207359), dense=0, sched=1)
    _has(_plan(plan_exe, 1920, 1080, cand=207360), dense=2, sched=0)
    _has(_plan(plan_exe, 1920, 1080, n=2, cand=207360, tiles=100), dense=0, sched=1)


def test_sparse_takes_over_at_12_active_tiles_and_the_list_from_4096_workgroups(plan_exe):
    _has(_plan(plan_exe, 1920, 1080, cand=50, tiles=12), sched=3, use_tile_list=0, listed_ok=0, may_sparse=1)
    _has(_plan(plan_exe, 1920, 1080, cand=50, tiles=12.5), sched=1, use_tile_list=0)
    _has(_plan(plan_exe, 1920, 1080, n=3, cand=50, tiles=100), listed_ok=1, sched=1, use_tile_list=1)   # 4368 >= 4096
    _has(_plan(plan_exe, 1920, 1080, n=2, cand=50, tiles=100), listed_ok=0, use_tile_list=0)            # 2912
    _has(_plan(plan_exe, 1920, 1080, n=3), listed_ok=1, dense=2, use_tile_list=0)                       # dense batches are never listed
    _has(_plan(plan_exe, 1920, 1080, n=3, cand=50, tiles=1), sched=3, use_tile_list=0)                  # nor SPARSE ones
    _has(_plan(plan_exe, 3840, 2160), listed_ok=1, may_sparse=1)                                        # 5768 alone; <= 8192
    _has(_plan(plan_exe, 7680, 4320), may_sparse=0)                                                     # 112 x 206 = 23072 tiles
    _has(_plan(plan_exe, 7680, 4320, cand=50, tiles=1), sched=1, use_tile_list=1)


def test_exact_arithmetic(plan_exe):
    """(the issue's table had threads 1024 here; the driver's rule is min(tuning or 512, 1024 for EXACT / 512 for
    FAST), so without tuning EXACT runs 512 threads too, and 1024 only when the tuning asks for them)"""
    _has(_plan(plan_exe, 1920, 1080, math=EXACT, cand=50, tiles=100), threads=512, dense=1, sched=0, listed_ok=0, dense128=0, use_tile_list=0)
    _has(_plan(plan_exe, 1920, 1080, math=EXACT, cand=50, tiles=12), sched=3, dense=1)
    _has(_plan(plan_exe, 1920, 1080, math=EXACT, threads=1024), threads=1024)
    _has(_plan(plan_exe, 1920, 1080, math=FAST, threads=1024), threads=512)
    _has(_plan(plan_exe, 1920, 1080, math=FAST, threads=256), threads=256)
    _has(_plan(plan_exe, 120, 68, n=9, math=EXACT), small_dense_ok=0, small_dense=0)
    for m in (capi.MATH_EXACT_FMA, capi.MATH_REF_FASTMATH, capi.MATH_REF_TEX8, capi.MATH_REF_TEX8_TRUNC):  # the diagnostic builds are EXACT's
        _has(_plan(plan_exe, 1920, 1080, math=m, n=3, cand=50, tiles=100), dense=1, listed_ok=0)


def test_forced_schedules(plan_exe):
    _has(_plan(plan_exe, 1920, 1080, mode=SPLIT, cand=0, tiles=0), sched=2, step=0, needs_ws=1, forced_split=1, may_split=0, parts=8)
    _has(_plan(plan_exe, 1920, 1080, mode=STEP, cand=0, tiles=0), sched=2, step=1, needs_ws=1, forced_split=1)
    _has(_plan(plan_exe, 1920, 1080, mode=PASS, cand=0, tiles=0, token=True), sched=4, step=0, needs_ws=1, want_pass=1, forced_split=1)
    _has(_plan(plan_exe, 1920, 1080, mode=PASS, cand=0, tiles=0, token=False), sched=2, step=1, want_pass=1)
    _has(_plan(plan_exe, 1920, 1080, mode=STEP, token=True), want_pass=0)
    _has(_plan(plan_exe, 1920, 1080, mode=STEP, parts=4), parts=4)
    # TILE: never split, never SPARSE, whatever the counters
    _has(_plan(plan_exe, 120, 68, mode=TILE), sched=0, dense=1, needs_ws=0, may_sparse=0, want_pass=0, forced_split=0)
    _has(_plan(plan_exe, 120, 68, mode=TILE, cand=10, tiles=1), sched=1)
    # SPARSE: every lean batch, whatever the number of active tiles; the dense first batch is TILE's
    _has(_plan(plan_exe, 1920, 1080, mode=SPARSE, cand=50, tiles=500), sched=3)
    _has(_plan(plan_exe, 1920, 1080, mode=SPARSE), sched=0, listed_ok=0)
    # the tests' hook: a forced TILE schedule with parts given lists from `parts` workgroups on
    _has(_plan(plan_exe, 240, 135, n=4, mode=TILE, parts=100, cand=10, tiles=100), listed_ok=1, use_tile_list=1)  # 112 >= 100
    _has(_plan(plan_exe, 240, 135, n=3, mode=TILE, parts=100, cand=10, tiles=100), listed_ok=0)                  # 84
    _has(_plan(plan_exe, 240, 135, n=4, mode=AUTO, parts=100, cand=10, tiles=100), listed_ok=0)


def test_pass_switches_and_latch(plan_exe):
    _has(_plan(plan_exe, 120, 68, mode=PASS), pass_switches=0)
    _has(_plan(plan_exe, 120, 68, mode=PASS, parts=1), pass_switches=1)
    _has(_plan(plan_exe, 120, 68, mode=PASS, parts=2), pass_switches=4)
    _has(_plan(plan_exe, 120, 68, mode=PASS, parts=1, test_timeout=1), pass_switches=3)
    _has(_plan(plan_exe, 120, 68, mode=PASS, parts=2, test_timeout=1), pass_switches=6)
    _has(_plan(plan_exe, 120, 68, mode=AUTO, parts=1, test_timeout=1), pass_switches=2)
    _has(_plan(plan_exe, 120, 68, latched=1, token=True), want_pass=0)
    _has(_plan(plan_exe, 120, 68, latched=1, mode=PASS, token=True), want_pass=1, sched=4)


def test_each_switch_flips_its_field(plan_exe):
    _has(_plan(plan_exe, 120, 68, no_pass=1), want_pass=0)
    _has(_plan(plan_exe, 120, 68, mode=PASS, no_pass=1), want_pass=0, needs_ws=1)
    _has(_plan(plan_exe, 960, 540, dense128=0), dense128=0, dense=1)
    _has(_plan(plan_exe, 480, 270, dense128=1), dense128=1, dense=2)
    _has(_plan(plan_exe, 960, 540, math=EXACT, dense128=1), dense128=0)
    _has(_plan(plan_exe, 1920, 1080, cand=50, tiles=1, tile_dense=1), dense=2, sched=0)
    _has(_plan(plan_exe, 1920, 1080, cand=50, tiles=0.5, sparse_tiles=0), sched=1)
    _has(_plan(plan_exe, 1920, 1080, cand=50, tiles=0, sparse_tiles=0), sched=3)
    _has(_plan(plan_exe, 1920, 1080, cand=50, tiles=40, sparse_tiles=40), sched=3)
    _has(_plan(plan_exe, 120, 68, step_max_tiles=0), may_split=0, needs_ws=0, sched=0, want_pass=1)
    _has(_plan(plan_exe, 480, 270, step_max_tiles=91), may_split=1, needs_ws=1, sched=2, parts=8)
    _has(_plan(plan_exe, 240, 135, cand=150, step_min_cand=150), sched=2)
    _has(_plan(plan_exe, 120, 68, n=9, no_corun=1), small_dense_ok=0, small_dense=0)
    _has(_plan(plan_exe, 1920, 1080, n=3, cand=50, tiles=100, no_tile_list=1), listed_ok=0, use_tile_list=0)


def test_switches_come_from_the_environment(plan_exe):
    def env_switches(**env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("VM_")}
        e.update(env)
        out = subprocess.run([plan_exe, "--env"], env=e, capture_output=True, text=True, check=True).stdout.split()
        return {k: float(v) for k, v in (f.split("=") for f in out)}
    assert env_switches() == dict(step_max_tiles=64, step_big_parts=8, corun_min_wgs=384, tile_list_min=4096, pass_max_groups=8,
                                  sparse_tiles=12, step_min_cand=200, no_corun=0, no_tile_list=0, no_pass=0, tile_dense=0, dense128=-1)
    got = env_switches(VM_STEP_MAX_TILES="0", VM_STEP_MIN_CAND="150.5", VM_SPARSE_TILES="3", VM_NO_CORUN="1", VM_NO_TILE_LIST="1",
                       VM_NO_PASS="1", VM_TILE_DENSE="1", VM_DENSE128="0")
    assert got == dict(step_max_tiles=0, step_big_parts=8, corun_min_wgs=384, tile_list_min=4096, pass_max_groups=8,
                       sparse_tiles=3, step_min_cand=150.5, no_corun=1, no_tile_list=1, no_pass=1, tile_dense=1, dense128=0)
    assert env_switches(VM_DENSE128="7")["dense128"] == 1
