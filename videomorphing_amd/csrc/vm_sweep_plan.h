// vm_sweep_plan.h -- which of the five sweep schedules (TILE dense / TILE lean / STEP or SPLIT / SPARSE / PASS) a
// batch of iterations runs, as pure functions of the call's geometry, the tuning, the environment switches and the
// previous batch's counters.  No HIP here: plain g++ compiles this header (tests/test_sweep_plan.py); the driver
// that acts on the plans is vm_sweep_sched.cpp.
#ifndef VM_SWEEP_PLAN_H
#define VM_SWEEP_PLAN_H

#include <algorithm>
#include <cstdlib>
#include <stdint.h>
#include "../../include/vmorph.h"

// The pitch of the sweep's tiles (vm_internal.h, where the whole tile geometry is explained).  Repeated here, not
// moved: vm_internal.h is part of the fingerprint of the sweep kernels' sources that the committed traffic profile
// carries, and the values are part of the algorithm's definition.  A unit that includes both headers has the
// preprocessor compare the two definitions.
#define VM_PITCH_X 69
#define VM_PITCH_Y 21

#ifndef VM_STEP_MAX_TILES
#define VM_STEP_MAX_TILES 64 // AUTO: levels of a batch with at most this many tiles per pass may run STEP
#endif
#ifndef VM_STEP_BIG_PARTS
#define VM_STEP_BIG_PARTS 8
#endif
#ifndef VM_CORUN_MIN_WGS
#define VM_CORUN_MIN_WGS 384 // small-level dense workgroups in flight on a device from which 256-thread workgroups pay (1.5 per CU)
#endif
#ifndef VM_TILE_LIST_MIN
#define VM_TILE_LIST_MIN 4096 // workgroups of a pruned TILE pass (tiles x pairs) from which the listed form pays
#endif
#ifndef VM_PASS_MAX_GROUPS
#define VM_PASS_MAX_GROUPS 8 // AUTO: PASS instead of STEP while a pass has at most this many tiles (x pairs): one 256-workgroup chunk
#endif
#ifndef VM_SPARSE_TILES
#define VM_SPARSE_TILES 12 // SPARSE takes a pruned level over once <= this many tiles per iteration were active
#endif
// dense TILE sweeps, FAST, 256-VGPR kernel: levels of at most this many tiles per pass run the form without the
// interior body.
// Levels of at most 32 tiles per pass (240x135 and below): most tiles touch the image border, so
// most tiles run the border form of the dense line search in some of their waves and wait for
// them; the interior form beside it only doubles the code the CU's waves execute at once.
// Without it (the same bits: the border form computes the same window counts at run time), us per
// dense pass (r03, tools/dev_dense.py): 30 x 120x68 187.5 -> 183.6, 30 x 240x135 623 -> 604, 3 x 240x135
// 182 -> 175; on large levels the interior form is what most waves run (1080p x 8 pairs, before the
// fixed fan-out: 36.6 ms per pass with it, 50.5 without).  A rule on the level, never on the batch.
// (This form also has no lean bodies, see tile_sweep: a phase of <= 16 candidates takes the two-lane
// search, so against the general kernel its results move by FAST rounding -- the same for a pair
// alone and in a batch, since the form follows from the level.)
#ifndef VM_NOINT_MAX_TILES
#define VM_NOINT_MAX_TILES 32
#endif

// tiles (= workgroups of a TILE launch per pair) of one of the four offset passes over a w x h level
inline int vm_tiles_per_pass(int w, int h)
{
    return ((w + VM_PITCH_X - 1) / VM_PITCH_X) * ((h + VM_PITCH_Y - 1) / VM_PITCH_Y);
}

// [0] TILE dense kernel, [1] TILE lean kernel, [2] STEP / SPLIT, [3] SPARSE, [4] PASS: the index of
// vm_progress.sched_ms / sched_launches
enum SweepSched { SCHED_TILE_DENSE = 0, SCHED_TILE_LEAN = 1, SCHED_STEP = 2, SCHED_SPARSE = 3, SCHED_PASS = 4 };

// The thresholds of the policy and the environment's development switches over them.
struct SweepSwitches {
    int step_max_tiles = VM_STEP_MAX_TILES;   // VM_STEP_MAX_TILES in the environment overrides it
    int step_big_parts = VM_STEP_BIG_PARTS;
    int corun_min_wgs = VM_CORUN_MIN_WGS;
    int tile_list_min = VM_TILE_LIST_MIN;
    int pass_max_groups = VM_PASS_MAX_GROUPS;
    int sparse_tiles = VM_SPARSE_TILES;       // VM_SPARSE_TILES
    // AUTO: STEP / PASS while the previous batch searched at least this many pixels per iteration and pair (below it
    // the pruned TILE kernel or SPARSE take over); VM_STEP_MIN_CAND
    double step_min_cand = 200.0;
    bool no_corun = false;     // VM_NO_CORUN: never 256-thread workgroups for small dense levels
    bool no_tile_list = false; // VM_NO_TILE_LIST: never the listed form of pruned TILE passes
    bool no_pass = false;      // VM_NO_PASS=1 turns the PASS schedule off, forced or not
    bool tile_dense = false;   // VM_TILE_DENSE: the dense TILE kernel whatever the counters say, and no SPARSE
    int dense128 = -1;         // VM_DENSE128=0 / 1 forces the 128-VGPR dense kernel off / on; -1: by the level's size
    int dense_noint = -1;      // VM_DENSE_NOINT=0 / 1: never / always the dense kernel without the interior form; -1: by the level's size

    // the process' switches, read from the environment once
    static const SweepSwitches &from_environment()
    {
        static const SweepSwitches sw = [] {
            SweepSwitches s;
            if (const char *e = getenv("VM_STEP_MAX_TILES")) s.step_max_tiles = atoi(e);
            if (const char *e = getenv("VM_STEP_MIN_CAND")) s.step_min_cand = atof(e);
            if (const char *e = getenv("VM_SPARSE_TILES")) s.sparse_tiles = atoi(e);
            s.no_corun = getenv("VM_NO_CORUN") != nullptr;
            s.no_tile_list = getenv("VM_NO_TILE_LIST") != nullptr;
            s.no_pass = getenv("VM_NO_PASS") != nullptr;
            s.tile_dense = getenv("VM_TILE_DENSE") != nullptr;
            if (const char *e = getenv("VM_DENSE128")) s.dense128 = atoi(e) != 0;
            if (const char *e = getenv("VM_DENSE_NOINT")) s.dense_noint = atoi(e) != 0;
            return s;
        }();
        return sw;
    }
};

// What a call of the driver is asked to do: the level's geometry, the pairs swept together, the context's settings.
struct SweepCall {
    int w = 0, h = 0, n = 1;
    int math_mode = VM_MATH_EXACT;
    int sweep_mode = VM_SWEEP_AUTO, sweep_threads = 0, sweep_parts = 0; // vm_set_tuning; 0 = automatic
    bool pass_latched_off = false;  // AUTO: a tile barrier timed out once on this context
    bool pass_test_timeout = false; // vm_dbg_pass_force_timeout is armed
};

// What holds for the whole call.
struct SweepLevelPlan {
    int tiles = 0;   // per pass and pair
    int groups = 0;  // tiles x pairs: the workgroups of a TILE launch, the tile groups of a PASS launch
    // FAST kernels are built for at most 512 threads (256-VGPR budget: the register-cached window sums must not
    // spill), EXACT ones for up to 1024
    int threads = 512;
    int parts = 8;               // SPLIT / STEP: workgroups per tile
    bool exact = false;          // EXACT and its diagnostic builds: every arithmetic but FAST
    bool forced_split = false;   // SPLIT, STEP or PASS is forced: every batch runs one of them
    bool two_kernel = false;     // ... and it is the two-kernel SPLIT (STEP's reference in the tests)
    bool may_split = false;      // AUTO may run STEP / PASS batches on this level
    bool needs_ws = false;       // the levels need the SPLIT / STEP workspace, and their old records forgotten
    bool may_sparse = false;
    bool forced_sparse = false;
    bool listed_ok = false;      // pruned TILE passes may take the listed form
    bool small_dense_ok = false; // dense TILE batches register with SmallDensePresence
    bool dense128 = false;
    bool dense_noint = false;    // a dense batch that is not the 128-VGPR form runs the form without the interior body
    bool tile_dense = false;     // (the switch)
    bool want_pass = false;      // before the device has been asked: resident workgroups, the token
    int pass_switches = 0;
    int corun_min_wgs = VM_CORUN_MIN_WGS;
    double split_min_cand = 0;   // AUTO splits while the previous batch's line searches per iteration reach this
    double lean_max_cand = 0;    // the lean regime: fewer line searches per iteration than this
    double sparse_max_tiles = 0;
};

struct SweepBatchPlan {
    SweepSched sched = SCHED_TILE_DENSE;
    int dense = 1;              // TILE / SPARSE: 0 the lean kernel, 1 the dense one, 2 its 128-VGPR form
    bool no_interior = false;   // TILE, dense == 1: the form without the interior body (VM_NOINT_MAX_TILES)
    bool step = false;          // sched == SCHED_STEP: one launch per phase (else the two-kernel SPLIT)
    bool use_tile_list = false; // TILE lean: the listed form
    bool small_dense = false;   // this batch launches small-level dense workgroups (SmallDensePresence)

    // the `dense` argument of the TILE launcher: `dense`, or 3 for the dense kernel without the interior body
    int tile_form() const { return no_interior ? 3 : dense; }
};

inline SweepLevelPlan plan_level(const SweepCall &q, const SweepSwitches &sw)
{
    SweepLevelPlan p;
    const int mode = q.sweep_mode;
    p.tiles = vm_tiles_per_pass(q.w, q.h);
    p.groups = p.tiles * q.n;
    p.exact = q.math_mode != VM_MATH_FAST;
    p.threads = std::min(q.sweep_threads ? q.sweep_threads : 512, p.exact ? 1024 : 512);
    // SPARSE: one workgroup per pair walks the few active tiles of a pruned level on the device
    p.forced_sparse = mode == VM_SWEEP_SPARSE;
    p.may_sparse = (mode == VM_SWEEP_AUTO || mode == VM_SWEEP_SPARSE) && p.tiles <= 8192;
    // Schedule, re-decided per batch of iterations (AUTO).  TILE: 4 launches per iteration, a
    // tile's four phases inside one workgroup -- unbeatable when a pass touches nothing (24 us
    // per converged iteration) or when there are enough tiles to fill the chip.  STEP (SPLIT
    // when forced): a tile's line searches spread over `parts` workgroups, 16 (32) launches
    // per iteration -- measured on MI355X (FAST, 1080p pyramid): 120x68, every pixel active,
    // 0.32 (STEP) vs 0.64 ms (TILE) per iteration; 240x135 with 900 line searches per
    // iteration 0.22 vs 0.36; with 90: 0.24 vs 0.23; converged 0.08 vs 0.024.  All schedules
    // work on the same state in HBM, so the choice can change from batch to batch.
    // (r03: restricting levels of more than 12 tiles per pass -- 240x135 -- to single pairs helped two
    // streams x 2 independent pairs, 274 -> 206 ms per job, and cost the coupled 5-frame video, whose
    // chain steps are batches of two pages, 354 -> 417 ms: not done)
    p.forced_split = mode == VM_SWEEP_SPLIT || mode == VM_SWEEP_STEP || mode == VM_SWEEP_PASS;
    p.two_kernel = mode == VM_SWEEP_SPLIT;
    p.may_split = mode == VM_SWEEP_AUTO && p.groups <= sw.step_max_tiles;
    p.needs_ws = p.forced_split || p.may_split;
    p.split_min_cand = sw.step_min_cand * q.n;
    // SPLIT / STEP schedules: workgroups per tile (every candidate gets 32 lanes, 16 candidates
    // per 512-thread workgroup)
    // (16 workgroups of 16 candidates per tile while the chip has room for them; 8 of 32 when a
    // phase-step of the batch would otherwise need more than two full waves of workgroups --
    // measured on 8 x 120x68: 232 -> 217 ms per level; 4 x 64 is slower again)
    // 32 on the smallest levels: with <= 8 candidates per workgroup k_step gives every
    // candidate a whole wave and its line search takes two steps per round (decide64) --
    // 120x68: 107 -> 98.5 ms per 500 iterations; 240x135 (28 tiles) is better off at 16.
    p.parts = q.sweep_parts ? q.sweep_parts : (p.groups * 16 >= 1024 ? sw.step_big_parts : (p.groups <= 12 ? 32 : 16));
    // (see SmallDensePresence, vm_sweep_sched.cpp) 256-thread workgroups only for the kernel the rule was measured
    // with: FAST, <= 32 tiles per pass, the automatic workgroup size
    p.small_dense_ok = !p.exact && !sw.no_corun && p.tiles <= 32 && q.sweep_threads == 0;
    p.corun_min_wgs = sw.corun_min_wgs;
    // (k_tile_scan) the listed form of pruned TILE passes: from VM_TILE_LIST_MIN workgroups per pass on, tiles that fit the
    // entries' 16 bits; counters and stamps start from zero in every call (the epochs do).  A forced TILE schedule with
    // parts given lowers the threshold to `parts` workgroups (tests)
    p.listed_ok = !p.exact && !sw.no_tile_list && (mode == VM_SWEEP_AUTO || mode == VM_SWEEP_TILE) &&
                  (size_t)p.tiles * q.n >= (size_t)(mode == VM_SWEEP_TILE && q.sweep_parts ? q.sweep_parts : sw.tile_list_min) &&
                  p.tiles <= 65535 && q.n <= 65535;
    // TILE, FAST arithmetic: the register-light kernel variant once fewer than a tenth of the pixels
    // are searched per iteration (after the first sweep of a level, typically)
    p.lean_max_cand = 0.1 * q.w * q.h * q.n;
    // dense sweeps, FAST: the 128-VGPR form of the dense kernel (>= 4 lanes per candidate, two
    // workgroups per CU) on levels of >= 256 tiles per pass (960x540 and up) -- measured on MI355X
    // (r03, tools/dev_dense.py, us per dense pass, 256- vs 128-VGPR kernel, with the taps shared by
    // lane pairs): 1080p x 1 pair 1399 vs 1290; 960x540 x 1 468 vs 466, x 8 2711 vs 2362, x 30 9946 vs
    // 8272; but 480x270 x 1 228 vs 306, x 8 726 vs 798 (x 30 2509 vs 2254), 240x135 x 30 875 vs 960,
    // 120x68 x 30 277 vs 438: with about one workgroup per CU the second round of a 256-candidate
    // phase costs more than the second workgroup hides.  The rule looks at the level only, never
    // at the batch: a pair is solved by the same kernels alone and in a batch (FAST sums are
    // ordered by the lane fan-out).  VM_DENSE128=0 / 1 forces it (dev switch).
    p.dense128 = !p.exact && (sw.dense128 >= 0 ? sw.dense128 != 0 : p.tiles >= 256);
    // (VM_NOINT_MAX_TILES) VM_DENSE_NOINT=0 / 1 forces it (dev switch)
    p.dense_noint = !p.exact && (sw.dense_noint >= 0 ? sw.dense_noint != 0 : p.tiles <= VM_NOINT_MAX_TILES);
    p.tile_dense = sw.tile_dense;
    p.sparse_max_tiles = (double)sw.sparse_tiles;
    // PASS: the workgroups of a tile group spin at a barrier of their own, so every group of a
    // launch must become resident whatever else runs.  One 256-workgroup chunk (8 groups) always
    // fits an idle MI355X; two PASS launches at once could starve each other's groups, so a
    // device-wide token (PassToken: across contexts AND processes) admits one holder at a time --
    // the others run STEP -- and the barrier's spin is bounded: in AUTO a timeout (a device whose
    // compute units are masked or otherwise not all ours) puts the level back to where the batch
    // started, reruns the batch with STEP and keeps this context off PASS from then on; only a
    // FORCED PASS schedule reports it as VM_E_DEVICE.  VM_NO_PASS=1 (environment) turns PASS off.
    p.want_pass = !sw.no_pass && (mode == VM_SWEEP_PASS ||
                                  (mode == VM_SWEEP_AUTO && !q.pass_latched_off && p.groups <= sw.pass_max_groups));
    // diagnostic forms of a FORCED PASS schedule (vm_set_tuning(VM_SWEEP_PASS, 0, parts)): parts == 1 stores
    // write-through from the start, parts == 2 maps 32 consecutive workgroup ids to a tile group, so that
    // every group spans all XCDs and takes the census -> write-back -> write-through route for real
    p.pass_switches = (mode == VM_SWEEP_PASS && q.sweep_parts == 1 ? 1 : 0) | (q.pass_test_timeout ? 2 : 0) |
                      (mode == VM_SWEEP_PASS && q.sweep_parts == 2 ? 4 : 0);
    return p;
}

// cand_prev: line searches per iteration in the previous batch, tiles_prev: active tile visits per iteration and
// pair in it (first batch: 1e9 both, i.e. dense); may_pass: PASS is wanted, the device can hold it and this call
// has the device's token.
inline SweepBatchPlan plan_batch(const SweepLevelPlan &p, double cand_prev, double tiles_prev, bool may_pass)
{
    SweepBatchPlan b;
    const bool split = p.forced_split || (p.may_split && cand_prev >= p.split_min_cand);
    // one launch per pass (PASS) where it is admitted, else one per phase (STEP), unless
    // the two-kernel SPLIT is forced
    const bool pass = split && may_pass;
    b.step = split && !pass && !p.two_kernel;
    const bool lean_regime = cand_prev < p.lean_max_cand;
    b.dense = (p.exact || p.tile_dense || !lean_regime) ? (p.dense128 ? 2 : 1) : 0;
    b.no_interior = b.dense == 1 && p.dense_noint;
    // SPARSE replaces the TILE launches of a pruned level once at most three tiles per pass
    // and pair are still active (measured on MI355X, 1080p: a no-op TILE iteration costs
    // 4 x 3.4 us, a no-op SPARSE iteration 4 x ~0.3 us; with more active tiles than that the
    // one workgroup per pair serialises what the TILE grid runs side by side)
    const bool sparse = p.may_sparse && !split && lean_regime && !p.tile_dense &&
                        (p.forced_sparse || tiles_prev <= p.sparse_max_tiles);
    b.sched = pass ? SCHED_PASS : (split ? SCHED_STEP : (sparse ? SCHED_SPARSE : (b.dense ? SCHED_TILE_DENSE : SCHED_TILE_LEAN)));
    const bool tile = !split && !sparse;
    // pruned TILE passes of a big batch: the listed form (k_tile_scan) -- dispatching tiles x pairs workgroups that
    // find nothing costs ~4.7 ns each, 118 us per pass over 30 1080p pairs
    b.use_tile_list = p.listed_ok && b.dense == 0 && tile;
    // dense TILE sweeps of a small level as 256-thread workgroups when enough of them are in flight on the
    // device to pair up on the CUs (SmallDensePresence) -- registered only while the call's CURRENT batch launches
    // such workgroups: a call that runs PASS, STEP, SPARSE or pruned lean batches has none in flight and must not
    // make another context believe it has company (measured there: 256-thread workgroups without a partner cost 16 %)
    b.small_dense = p.small_dense_ok && b.dense == 1 && tile;
    return b;
}

#endif
