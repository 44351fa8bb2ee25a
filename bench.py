#!/usr/bin/env python
"""bench.py -- headline benchmark of the halfway-domain morph solver.

Metric (BASELINE.json): Mpixel*iters/s of the halfway optimizer.

  --config 1  (default at N = 1) config[1]: ONE 1920x1080 frame pair, 6-level pyramid
              (start_res 32), 500 iterations per level.  A step = one complete
              coarse-to-fine solve (vm_solve) of one pair whose pyramid is resident in HBM;
              every step solves a different frame of the synthetic video.
  --config 2  (default at N > 1) config[2]: 60 independent 1080p frame pairs sharded over
              the ranks (static block distribution, videomorphing_amd.dist.shard_pairs); a
              step = every rank solves ITS pairs as batches (vm_solve_batch: all pairs of a
              batch relaxed by the same launches).  Total work is fixed: strong scaling.
  --config 3  config[3]: one 3840x2160 pair, 7-level pyramid, otherwise as config 1.
  --config 4  config[4]: 30 1080p pairs with 8 point constraints each and BCOND_BORDER, block-sharded over the
              ranks like config 2; a step = every rank solves ITS pairs (vm_solve_batch_cons on its streams), extends
              both canvases of every pair (Poisson, batched) and renders nine in-between frames per pair on its
              compositor lanes.  The constraints ride in the ONE broadcast of the parameter block.  The line's
              value is rendered frames/s of the whole job (BASELINE's second metric), the solve stage's
              Mpixel*iters/s beside it under "pipeline".  `--as-rank k --of G` runs rank k's share alone.

value = sum over levels of W*H*EXECUTED iterations (the reference's own progress unit,
`_current_iter += W*H` per sweep that runs, morph.cu:1389: sweeps up to and including a level's
first without an accepted move) over all ranks / max-over-ranks wall time; value_nominal credits
max_iter sweeps per level whether they ran or not and is quoted beside it, never as the headline.  No collective sits on the data
path; the only exchanges are one RCCL broadcast of the parameter block and one all-gather of
two scalars per rank for the report.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the line (roofline figures from the timed steps and the
committed profiles).  --full adds what takes runs of its own: scale_reference, the extras (the other stopping rule and
arithmetic, batched, temporal, sync, compositor stages, config[3] and config[4] on one GPU) and cpu_baseline with its
bit-for-bit parity check.  --dump-outputs DIR writes what the last timed step computed (dump_outputs).
With N > 1 and no torch.distributed environment the script starts its N ranks itself (as
child processes, before anything touches the GPU); under
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` it is one rank.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

# The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues per device (default 4): a
# fifth stream shares a queue with another and their kernels serialise.  This script holds the context of its config[1]
# steps AND the three of `scale_reference` (plus torch's own stream): measured, 60 pairs on three streams 1312 ms with
# the default against 838 with 8 queues.  Set before anything initialises HIP; a host that runs more than three solver
# contexts per process should do the same.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

START_RES, MAX_ITER, DROP = 32, 500.0, 1.0
CONFIG_SIZE = {1: (1920, 1080), 2: (1920, 1080), 3: (3840, 2160), 4: (1920, 1080)}
ALG_BYTES_PER_VISIT = 100.0      # 76 B read + 24 B written per pixel-visit
FLOP_PER_EVAL = 25 * 45 + 2 * 30  # 25 ssim() of ~45 flop-eq + 2 bilinear taps of ~30
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: 8.0 TB/s spec
VALU_PEAK_FLOPS = 157e12         # MI355X_MICROARCH.md: f32 vector peak
POISSON_ALG_BYTES = 178.0        # algorithmic bytes per unknown and PCG iteration of the Poisson solver (190 until the PCG
POISSON_ALG_BYTES_FUSED = 178.0  # update moved into the level-0 restriction: the residual is no longer read twice)
from fullsize_fixture import POISSON_TIMED_TOLS      # noqa: E402  the tolerances the full-size oracle fixtures verify (<= 1 colour level)
POISSON_TOL = POISSON_TIMED_TOLS[0]
SCHED = ("k_optimize<true> (TILE schedule, dense kernel)", "k_optimize<false> (TILE schedule, lean kernel for pruned sweeps)",
         "k_step (STEP schedule, one launch per phase)",
         "k_sparse (SPARSE schedule: one launch per batch of iterations of a pruned level)",
         "k_pass (PASS schedule: one launch per pass, the four phases of a tile behind tile-local barriers)")
# kernel-name prefixes of each schedule in the PMC summaries (template variants of one schedule are
# combined, weighted by their launches in the profiled run)
SCHED_PMC = ("k_optimize_fast<true", "k_optimize_fast<false", "k_step_fast", "k_sparse_fast<", "k_pass_fast")
NSCHED = 5
# launches per iteration of each schedule (a SPARSE launch covers a batch of iterations)
SCHED_LAUNCHES_PER_ITER = (4.0, 4.0, 16.0, None, 4.0)


def tile_visits(w, h):
    """pixel-visits of the 4 tile-offset launches of one iteration (64x16 tiles, 69x21 pitch)"""
    def cover(dim, tile, pitch, off):
        n, t = 0, off
        while t < dim:
            n += min(tile, dim - t)
            t += pitch
        return n
    tot = 0
    for ox in (0, 64):
        for oy in (0, 16):
            tot += cover(w, 64, 69, ox) * cover(h, 16, 21, oy)
    return tot


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=0, choices=[0, 1, 2, 3, 4],
                    help="BASELINE.json config index; 0 = 1 on one GPU, 2 on several")
    ap.add_argument("--pairs", type=int, default=0, help="config 2 / 4: frame pairs of the whole job (0 = the config's own: 60 / 30)")
    ap.add_argument("--digest", default="", help="config 4, development / tests: write every rank's rendered frames' SHA-256 and its fields' to this "
                                                 "JSON file (rank k appends `.k`)")
    ap.add_argument("--max-batch", type=int, default=32, help="config 2: most pairs relaxed by one launch")
    ap.add_argument("--math", default="fast", choices=["fast", "exact"])
    ap.add_argument("--semantics", default="fixed", choices=["fixed", "reference"],
                    help="fixed: every level runs its max_iter sweeps (BASELINE config: 500 iters/level); "
                         "reference: a level stops when no pixel improved (morph.cu:1390)")
    ap.add_argument("--inflight", type=int, default=0,
                    help="HIP streams (contexts, one host thread each) per GPU working on different pairs at the same "
                         "time; 0 = 1 for config 1/3, 2 for config 2")
    ap.add_argument("--batch", type=int, default=1,
                    help="config 1/3: pairs solved together by the same sweep launches; a step is then one batch")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend of the two collectives: nccl = RCCL over xGMI (the product path); "
                         "gloo lets a box with fewer GPUs than ranks exercise the N > 1 code (ranks then share devices)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true")
    ap.add_argument("--no-extras-but-scale-ref", action="store_true", help="no extras except scale_reference")
    ap.add_argument("--no-scale-ref", action="store_true",
                    help="N = 1, config 1: skip `scale_reference` (config[2]'s job -- the workload an N > 1 run shards -- on this one GPU)")
    ap.add_argument("--scale-ref-pairs", type=int, default=60, help="frame pairs of the scale_reference job")
    ap.add_argument("--extras", default="", help="development: comma-separated names of the extras to run (default: all): semantics, "
                                                 "math, batched, temporal, sync, render, poisson, qpath, pipeline8, pipeline30, config3")
    ap.add_argument("--scale-ref-last", action="store_true", help="development: run scale_reference AFTER the other extras (the order "
                                                                    "rounds 3-4 found 16 %% slower; profiles/r05_notes.md section 7)")
    ap.add_argument("--size", default=None, help="WxH override (development only)")
    ap.add_argument("--sweep-threads", type=int, default=0, help="threads per sweep workgroup, 0 = the library's choice (development only)")
    ap.add_argument("--sweep-parts", type=int, default=0, help="workgroups per tile of the STEP schedule, 0 = the library's choice (development only)")
    ap.add_argument("--as-rank", type=int, default=-1,
                    help="config 2 on ONE GPU: solve the shard rank K of an --of G-rank job would get (static partition "
                         "study: per-rank load without the G GPUs)")
    ap.add_argument("--of", type=int, default=8)
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: scale_reference, the extras (other semantics, "
                         "arithmetic, sizes, stages and configurations) and the cpu_baseline leg with its parity check; "
                         "--no-extras, --no-scale-ref, --no-cpu-baseline and --extras select among them")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / "
                         "float64, at most 64 MB in all: a fixed, seeded sample of a larger output); rank k > 0 of an "
                         "N > 1 run writes <name>_rank<k>.npy")
    return ap.parse_args(argv)


def main():
    args = parse_args()
    # ---- N > 1 asked for from a plain invocation: become the launcher (no GPU call, no torch) ----
    from videomorphing_amd import launch
    if launch.needs_launch(args.gpus):
        sys.exit(launch.self_launch(os.path.abspath(__file__), sys.argv[1:], args.gpus))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE is %d: start it as `python bench.py --gpus N` or under "
                         "torch.distributed.run with --nproc-per-node equal to --gpus" % (args.gpus, world))
    config = args.config or (1 if world == 1 else 2)
    if args.pairs <= 0:
        args.pairs = 30 if config == 4 else 60
    w, h = CONFIG_SIZE[config]
    if args.size:
        w, h = [int(x) for x in args.size.lower().split("x")]

    import numpy as np
    import torch
    import torch.distributed as dist
    if args.backend == "gloo":
        # test mode: ranks may share a device.  Nothing to configure for that: the PASS schedule's token is a
        # per-device lock file (one holder at a time across processes, the others run STEP), vm_api.cpp
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    coll_dev = torch.device("cuda", local_rank) if args.backend == "nccl" else torch.device("cpu")
    if world > 1:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=coll_dev)
        else:
            dist.init_process_group("gloo")

    from videomorphing_amd import capi, morph, synth
    from videomorphing_amd import dist as vdist

    # ---- the shared parameter block: rank 0 decides, one RCCL broadcast ----
    blk = capi.ParamBlock()
    if rank == 0:
        P = morph.Parameters()
        blk.kp = morph.KernParameters(P)
        blk.max_iter, blk.max_iter_drop_factor, blk.start_res = MAX_ITER, DROP, START_RES
        blk.math_mode = capi.MATH_FAST if args.math == "fast" else capi.MATH_EXACT
    # (config[4]: the frames' point constraints are part of the block -- they travel in the same one broadcast)
    raw = vdist.pack_block(blk, synth.make_constraints(w, h, 8) if (rank == 0 and config == 4) else None)
    if world > 1:
        # backend "nccl" is RCCL on ROCm (xGMI within the node)
        raw = vdist.broadcast_block(raw, coll_dev)
    blk, _cons = vdist.unpack_block(raw)
    if config == 4:
        config4_main(args, np, torch, dist, vdist, capi, morph, synth, blk, _cons, rank, local_rank, world, coll_dev, w, h)
        return

    # config 2: two streams per GPU by default -- measured on MI355X (profiles/r03_notes.md, 8 / 60 pairs
    # on one GPU): 1 stream 21.3 / 38.2, 2 streams 25.3 / 47.9, 4 streams 20.2 / 46.2 G pixel*iters/s
    # (beyond two the host's launch rate, ~3.5 us per eager launch under the runtime's lock, binds) --,
    # three from 24 pairs per GPU on (r04, ms per job, 2 -> 3 streams: 60 pairs 859 -> 838, 30 pairs 569 -> 558,
    # 15 pairs 466 -> 479)
    if config == 2 and args.inflight == 0:
        my_pairs = len(vdist.shard_pairs(args.pairs, world, rank) if args.as_rank < 0 else vdist.shard_pairs(args.pairs, args.of, args.as_rank))
        args.inflight = default_streams(my_pairs)
    nctx = max(1, args.inflight)
    # (development: VM_DEV_DUMMY_STREAMS=k idle contexts created first shift which hardware queues the runtime deals the
    #  solver streams to -- tools/exp/rep_shard.sh, profiles/r06_notes.md section 4)
    _dummies = [morph.Context(local_rank, blk.math_mode) for _ in range(int(os.environ.get("VM_DEV_DUMMY_STREAMS", "0")))]
    ctxs, streams_rejected = solver_contexts(morph, local_rank, blk.math_mode, nctx)
    if os.environ.get("VM_DEV_DUMMY_STREAMS") and nctx > 1:
        print("solver streams side by side (vm_dbg_streams_overlap):", [(i, j, ctxs[i].runs_beside(ctxs[j])) for i in range(nctx) for j in range(i + 1, nctx)],
              "rejected on the way:", streams_rejected, file=sys.stderr)
    for c in ctxs:
        c.set_params(blk.kp)
        if args.sweep_threads or args.sweep_parts:
            c.set_tuning(capi.SWEEP_AUTO, args.sweep_threads, args.sweep_parts)
    ctx = ctxs[0]
    L = capi.load()
    nlev = synth.num_levels(w, h, blk.start_res)
    FIXED = 1 if args.semantics == "fixed" else 0

    # ---- inputs: pyramids resident in HBM before the timed region ----
    def frames(ids):
        from concurrent.futures import ThreadPoolExecutor
        # (the ranks of one node share its cores: each takes its share)
        with ThreadPoolExecutor(max_workers=max(1, min(effective_cpus() // max(world, 1), 16, len(ids)))) as ex:   # numpy releases the GIL
            return list(ex.map(lambda f: synth.make_pair(w, h, frame=f), ids))

    def pyramid(c, imgs):
        p = morph.Pyramid(c)
        p.build(imgs[0], imgs[1], blk.start_res, nlevels=nlev)
        return p

    distinct_frames = None
    if config == 2:
        mine = vdist.shard_pairs(args.pairs, world, rank) if args.as_rank < 0 else vdist.shard_pairs(args.pairs, args.of, args.as_rank)
        pyrs, B, nctx, distinct_frames = config2_setup(mine, ctxs, frames, pyramid, args.max_batch)
        step_sets = [pyrs] * (args.steps + args.warmup)       # every step re-solves the rank's shard
    else:
        B = max(1, args.batch)
        npairs = (args.steps + args.warmup) * B
        ids = [rank * npairs + k for k in range(npairs)]
        imgs = frames(ids)
        pyrs = [pyramid(ctxs[(k // B) % nctx], imgs[k]) for k in range(npairs)]
        step_sets = [pyrs[s * B:(s + 1) * B] for s in range(args.steps + args.warmup)]
    sizes = [(pyrs[0][el].width, pyrs[0][el].height) for el in range(1, nlev + 1)]

    def solve(p, fixed=FIXED):
        prog = (capi.Progress * (nlev - 1))()
        capi.check(L.vm_solve(p._h, blk.max_iter, blk.max_iter_drop_factor, None, 0, None, fixed, prog))
        return prog

    def solve_group(ps, fixed=FIXED):
        """a batch of pairs relaxed by the same launches"""
        if len(ps) == 1:
            return [solve(ps[0], fixed)]
        arr = (C.c_void_p * len(ps))(*[p._h for p in ps])
        prog = (capi.Progress * (len(ps) * (nlev - 1)))()
        capi.check(L.vm_solve_batch(arr, len(ps), blk.max_iter, blk.max_iter_drop_factor, None, fixed, prog))
        out = []
        for i in range(len(ps)):
            one = (capi.Progress * (nlev - 1))(*[prog[i * (nlev - 1) + k] for k in range(nlev - 1)])
            if i > 0:          # elapsed/launches are per batch: count them once
                for k in range(nlev - 1):
                    one[k].elapsed_ms, one[k].launches = 0.0, 0
                    for j in range(NSCHED):
                        one[k].sched_ms[j], one[k].sched_launches[j] = 0.0, 0
            out.append(one)
        return out

    def run_step(ps):
        """one step; with several contexts, one host thread per context (a vm_ctx is
        single-threaded by contract)"""
        if config == 2:
            return config2_step(ps, ctxs[:nctx], B, solve_group)
        if B > 1:
            out = []
            for g0 in range(0, len(ps), B):
                out += solve_group(ps[g0:g0 + B])
            return out
        return [solve(p) for p in ps]

    def run_steps(sets):
        if nctx > 1 and B == 1 and config != 2:
            from concurrent.futures import ThreadPoolExecutor
            flat = [p for ps in sets for p in ps]
            groups = {}
            for i, p in enumerate(flat):
                groups.setdefault(id(p._ctx), []).append((i, p))
            out = [None] * len(flat)

            def work(items):
                for i, p in items:
                    out[i] = solve(p)
            with ThreadPoolExecutor(max_workers=len(groups)) as ex:   # ctypes calls release the GIL
                list(ex.map(work, groups.values()))
            return out, []
        out, per_step = [], []
        for ps in sets:
            t1 = time.perf_counter()
            out += run_step(ps)
            for c in ctxs:
                c.sync()
            per_step.append((time.perf_counter() - t1) * 1e3)
        return out, per_step

    def sync_all():
        for c in ctxs:
            c.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    run_steps(step_sets[:args.warmup])
    sync_all()
    t0 = time.perf_counter()
    progs, step_ms = run_steps(step_sets[args.warmup:])
    for c in ctxs:
        c.sync()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    sync_all()

    R = range(nlev - 1)
    pix_iters = sum(pr[i].pixel_iters for pr in progs for i in R)
    # ... of which executed: iterations up to and including a level's first without an accepted
    # move (what the reference's loop runs); the rest of a fixed-work level are skipped no-ops
    pix_live = sum(float(pr[i].iters_live) * sizes[i][0] * sizes[i][1] for pr in progs for i in R)
    if world > 1:
        el_max, pix_total, pix_live_total = vdist.reduce_report(el, pix_iters, coll_dev, pix_live)
    else:
        el_max, pix_total, pix_live_total = el, pix_iters, pix_live

    # (rounds 3-4 ran scale_reference first because after the other extras it took 970 instead of 838 ms.  Round 5 found the
    # cause -- profiles/r05_scale_ref_bisect.txt: the TEMPORAL extra, and in it the video lanes' graded stream priorities: their
    # low-priority streams took hardware queues the runtime never handed back, so two of the job's three streams then shared
    # one.  Fixed in vm_video.cpp (the lanes run on plain streams); the order no longer matters: 836 ms either way.)
    if args.dump_outputs:
        # what a caller of vm_solve / vm_solve_batch receives from the last timed step: every pair's full-resolution halfway
        # field and the sweeps each level executed (the timing fields of vm_progress are not outputs)
        last = step_sets[-1]
        dump_outputs(args.dump_outputs, {"v": np.stack([p[1].v for p in last]),
                                         "iters_executed_per_level": np.array([[pr[i].iters_live for i in range(nlev - 1)]
                                                                               for pr in progs[len(progs) - len(last):]], np.float64)},
                     rank if world > 1 else None)

    # everything below the headline (other workloads, configurations, the CPU leg) runs only with --full
    extras = {}
    scale_ref = None
    want_scale_ref = args.full and rank == 0 and world == 1 and config == 1 and not args.size and not (args.no_extras or args.no_scale_ref)
    if want_scale_ref and not args.scale_ref_last:
        scale_ref = scale_reference(args, morph, blk, local_rank, frames, solve_group, sizes, nlev, FIXED)
    if args.full and rank == 0 and not (args.no_extras or args.no_extras_but_scale_ref) and config != 2:
        extras = run_extras(args, np, capi, morph, synth, L, blk, ctx, pyrs[0], w, h, nlev, FIXED, B, solve, solve_group, local_rank, frames)
    if want_scale_ref and args.scale_ref_last:
        scale_ref = scale_reference(args, morph, blk, local_rank, frames, solve_group, sizes, nlev, FIXED)
    if scale_ref is not None:
        extras["scale_reference"] = scale_ref

    cpu = None
    if args.full and rank == 0 and not args.no_cpu_baseline:
        cpu = cpu_baseline(np, capi, L, blk, [p for p in pyrs[:3] if p._ctx is ctx], nlev, ctx)

    if rank == 0:
        out = report(args, config, world, w, h, nlev, blk, capi, B, nctx, FIXED, sizes, progs, step_ms, el_max, pix_total,
                     cpu, distinct_frames, len(pyrs) if config == 2 else None, pix_live_total,
                     frame_ids=ids[args.warmup * B:] if config != 2 else None)
        out.update(extras)
        # streams this rank created and gave back because they shared a hardware queue with another solver stream (solver_contexts)
        out["config"]["solver_streams_rejected_for_sharing_a_hardware_queue"] = streams_rejected
        if args.as_rank >= 0:
            out["as_rank"] = {"rank": args.as_rank, "of": args.of, "pairs": len(pyrs),
                              "note": "the shard this rank of the job would solve, run alone on one GPU"}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def config4_main(args, np, torch, dist, vdist, capi, morph, synth, blk, cons, rank, local_rank, world, coll_dev, w, h):
    """`--config 4`: this rank's share of the 30-pair job (Config4Job), W warm-up + K timed steps between barriers, max over
    ranks, one all-gather of a few scalars per rank, rank 0 prints the line."""
    import hashlib
    nlev = synth.num_levels(w, h, blk.start_res)
    ex = int(0.1 * max(w, h))                                    # pyramid.cu:194
    mine = vdist.shard_pairs(args.pairs, world, rank) if args.as_rank < 0 else vdist.shard_pairs(args.pairs, args.of, args.as_rank)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, min(effective_cpus() // max(world, 1), 16, max(len(mine), 1)))) as ex_:
        imgs = list(ex_.map(lambda f: synth.make_pair(w, h, frame=f), mine))
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    job = Config4Job(np, capi, morph, synth, local_rank, blk, cons, w, h, nlev, mine, imgs, rgb0, rgb1, ex, POISSON_TOL)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()
    try:
        group = job.pyramids()
        if mine:
            job.warm_up(group)
            for _ in range(args.warmup):
                job.step(group)
        barrier()
        t0 = time.perf_counter()
        runs = [job.step(group) for _ in range(args.steps)] if mine else []
        el = time.perf_counter() - t0
        barrier()
        if args.dump_outputs and runs:
            # the solve stage's result of the last timed step (every pair's halfway field) and the compositor's PCG
            # iteration counts; the rendered frames stay on the device in the timed path
            dump_outputs(args.dump_outputs, {"v": np.stack([q[1].v for q in group]), "pcg_iterations": np.array(runs[-1]["its"], np.float64)},
                         rank if world > 1 else None)
        if args.digest and mine:       # one more, untimed step whose frames and fields are fingerprinted (tests)
            got = {}
            job.step(group, collect=got)
            doc = {"pairs": mine, "frames": {}, "fields": {}, "frame_bytes": {}}
            for (k, what), a in sorted(got.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
                if what == "v":
                    doc["fields"][str(mine[k])] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
                else:
                    doc["frames"]["%d/%d" % (mine[k], what)] = hashlib.sha256(a.tobytes()).hexdigest()
                    if what == 5:
                        doc["frame_bytes"][str(mine[k])] = a[::16, ::16].tolist()
            json.dump(doc, open(args.digest + (".%d" % rank if world > 1 else ""), "w"))
        n = len(mine)
        frames_done = n * 9 * args.steps
        solve_s = sum(r["solve_s"] for r in runs)
        comp_s = sum(r["comp_s"] for r in runs)
        pix = sum(r["pixel_iters"] for r in runs)
        if world > 1:
            import torch as _t
            mine_t = _t.tensor([el, frames_done, pix, solve_s, comp_s, n], dtype=_t.float64, device=coll_dev)
            every = [_t.zeros_like(mine_t) for _ in range(world)]
            dist.all_gather(every, mine_t)
            per = _t.stack(every).cpu().numpy()
        else:
            per = np.asarray([[el, frames_done, pix, solve_s, comp_s, n]], dtype=np.float64)
        if rank == 0:
            el_max = float(per[:, 0].max())
            its = [i_ for r in runs for i_ in r["its"]]
            best = min(runs, key=lambda r: r["s"]) if runs else None
            out = {"metric": "rendered frames/s of the config[4] pipeline (constrained halfway solve + Poisson-extended boundary + warp/blend render); "
                             "Mpixel*iters/s of its solve stage under `pipeline`",
                   "value": round(float(per[:, 1].sum()) / el_max, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                   "ms_per_step": round(el_max * 1e3 / max(args.steps, 1), 2), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                   "dtype": "f32", "data": "synthetic",
                   "config": {"workload": config4_workload(args.pairs, job.nstreams, len(job.chunks(group)[0]) if mine else 0, ex, job.per_batch, job.nlanes, POISSON_TOL)
                                          + "; pairs block-sharded over %d rank(s), rank 0 holds %d" % (world if args.as_rank < 0 else args.of, n),
                              "pairs": args.pairs, "rendered_frames_per_pair": 9, "poisson_tol": POISSON_TOL,
                              "poisson_tol_verified_by": "tests/test_gpu_fullsize_compositor.py (oracle CG at 1e-9 on the 2304x1464 canvas: max |colour difference| <= 1)",
                              "math": "fast" if blk.math_mode == capi.MATH_FAST else "exact", "semantics": "reference (a level stops at its first sweep without an accepted move)",
                              "collectives": "one broadcast of the parameter block INCLUDING the %d point constraints (%d bytes), one all-gather of 6 scalars per rank" % (len(cons), 20 * len(cons))},
                   "pipeline": {"ms_per_pair_slowest_rank": round(el_max * 1e3 / max(args.steps, 1) / max(float(per[:, 5].max()), 1.0), 2),
                                "solve_mpix_iters_per_s": round(float(per[:, 2].sum()) / max(float(per[:, 3].max()), 1e-9) / 1e6, 1),
                                "per_rank": [{"pairs": int(r[5]), "s_per_step": round(r[0] / max(args.steps, 1), 4), "solve_s_per_step": round(r[3] / max(args.steps, 1), 4),
                                              "compositor_s_per_step": round(r[4] / max(args.steps, 1), 4)} for r in per],
                                "rank0": best and {"solve_ms_per_pair": round(best["solve_s"] * 1e3 / n, 2), "compositor_ms_per_frame": round(best["comp_s"] * 1e3 / n, 2),
                                                   "compositor_split_ms_per_frame": {"upload_pcie_and_v_upscale": round(best["split"][0] / n * 1e3, 2),
                                                                                     "poisson_both_sides": round(best["split"][1] / n * 1e3, 2),
                                                                                     "render_9_frames": round(best["split"][2] / n * 1e3, 2)},
                                                   "pcg_iterations_min_max": [min(its), max(its)] if its else None}},
                   "roofline": None, "cpu_baseline": None,
                   "note": "config[4] is not the configuration BASELINE's metric is quoted on (that is config[1], the default run): no roofline / cpu_baseline objects here; "
                           "the Poisson solver's roofline is in the default line's poisson_extend_1080p_ex192"}
            if args.as_rank >= 0:
                out["as_rank"] = {"rank": args.as_rank, "of": args.of, "pairs": n, "note": "the shard this rank of the job would process, run alone on one GPU"}
            print(json.dumps(out), flush=True)
    finally:
        job.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def config2_setup(mine, ctxs, frames, pyramid, max_batch):
    """config[2] on one rank: the rank's pairs `mine` as pyramids resident in HBM, in len(ctxs) contiguous
    chunks -- one context (HIP stream + host thread) each --, a chunk solved in even batches of <= max_batch
    pairs per launch.  Every pair is its own frame of the synthetic video (rounds 1-4 reused 8 frames cyclically:
    which of them cycle then set the executed units of the whole job).  Returns (pyrs, B, nctx, distinct)."""
    distinct = list(mine)
    imgs = frames(distinct)
    nctx = min(len(ctxs), max(1, len(mine)))
    chunk_of = [k * nctx // max(len(mine), 1) for k in range(len(mine))]
    pyrs = [pyramid(ctxs[chunk_of[k]], imgs[k % len(imgs)]) for k in range(len(mine))]
    per_ctx = (len(mine) + nctx - 1) // nctx
    B = max(1, min(max_batch, per_ctx))
    nb = (per_ctx + B - 1) // B
    B = (per_ctx + nb - 1) // nb              # even batches: 60 pairs on one GPU and stream = 2 x 30
    return pyrs, B, nctx, len(distinct)


def config2_step(ps, ctxs, B, solve_group):
    """one step of config[2] on one rank: every context's chunk in batches of B pairs, one host thread per
    context (a vm_ctx is single-threaded by contract; ctypes calls release the GIL)"""
    def work(chunk):
        res = []
        for g0 in range(0, len(chunk), B):
            res += solve_group(chunk[g0:g0 + B])
        return res
    chunks = [[p for p in ps if p._ctx is c] for c in ctxs]
    if len(ctxs) == 1:
        return work(chunks[0])
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(ctxs)) as ex:
        return [r for res in ex.map(work, chunks) for r in res]


def solver_contexts(morph, device, math_mode, n):
    """n contexts (HIP streams) for a job whose pairs are solved on several streams at once -- each one checked to run SIDE
    BY SIDE with those before it (morph.context_beside / vm_dbg_streams_overlap): the runtime deals a new stream to one of
    its GPU_MAX_HW_QUEUES hardware queues as it likes, and two solver streams that land on one queue take turns -- measured
    with idle streams created first to shift the deal (tools/exp/shard_dummy.sh): the 8-pair shard 519 instead of 329 ms, the
    60-pair job 1360 instead of 856 ms, and the probe names exactly those pairs.  A default run has never hit it; a rank of
    an N > 1 run (RCCL's own streams come first there) or a host with other streams alive may.  Returns (contexts, streams
    rejected on the way)."""
    ctxs, rejected = [], 0
    for _ in range(n):
        c, nrej = morph.context_beside(device, math_mode, ctxs)
        ctxs.append(c)
        rejected += nrej
    return ctxs, rejected


def default_streams(pairs_on_this_gpu):
    """streams (contexts, each driven by its own host thread) for config[2]'s job on one GPU"""
    return 3 if pairs_on_this_gpu >= 24 else 2


def clock_mhz(progs, R, which):
    """shader clock held inside a sweep kernel: the in-kernel probe's sum of s_memtime differences / sum of
    s_memrealtime differences x 100 MHz over every launch of the run (vm_progress.clk_*: [0] dense TILE kernel, [1] k_pass)"""
    c = sum(pr[i].clk_shader_ticks[which] for pr in progs for i in R)
    t = sum(pr[i].clk_wall_ticks[which] for pr in progs for i in R)
    return round(c / t * 100.0, 1) if t > 0 else None


def activity(progs, R, seconds, kern_ms):
    """energy evaluations / line searches per second of wall time and the VALU fraction SURVEY 8(d) defines
    (evaluations x 1185 flop-equivalents / HIP-event time of the sweep kernels / 157 TFLOP/s)"""
    evals = sum(pr[i].evaluations for pr in progs for i in R)
    ls = sum(pr[i].candidates for pr in progs for i in R)
    return {"evals_per_s": round(evals / seconds), "line_searches_per_s": round(ls / seconds),
            "valu_frac": round(evals * FLOP_PER_EVAL / (kern_ms * 1e-3) / VALU_PEAK_FLOPS, 5) if kern_ms > 0 else None}


def scale_reference(args, morph, blk, local_rank, frames, solve_group, sizes, nlev, fixed):
    """The workload an N > 1 run of this script shards (config[2]: --scale-ref-pairs independent 1080p
    pairs, the streams of default_streams(), batches of <= --max-batch pairs per launch) on THIS one GPU: the same-workload
    denominator of a scaling curve whose N = 1 point is config[1].  Never fatal: a failure (a smaller or shared GPU
    running out of memory, say) is reported in place of the figures and the headline line is printed all the same."""
    ctxs, pyrs = [], []
    try:
        ctxs, _ = solver_contexts(morph, local_rank, blk.math_mode, default_streams(args.scale_ref_pairs))
        for c in ctxs:
            c.set_params(blk.kp)

        def pyramid(c, imgs):
            p = morph.Pyramid(c)
            p.build(imgs[0], imgs[1], blk.start_res, nlevels=nlev)
            return p
        mine = list(range(args.scale_ref_pairs))
        pyrs, B, nctx, distinct = config2_setup(mine, ctxs, frames, pyramid, args.max_batch)
        config2_step(pyrs, ctxs[:nctx], B, solve_group)                    # warm-up (workspaces, graphs)
        for c in ctxs:
            c.sync()
        t0 = time.perf_counter()
        progs = config2_step(pyrs, ctxs[:nctx], B, solve_group)
        for c in ctxs:
            c.sync()
        dt = time.perf_counter() - t0
        R = range(nlev - 1)
        nominal = sum(pr[i].pixel_iters for pr in progs for i in R)
        live = sum(float(pr[i].iters_live) * sizes[i][0] * sizes[i][1] for pr in progs for i in R)
        # sweep-kernel time summed over the streams: they overlap, so the VALU fraction is quoted against the WALL time
        kern_ms = sum(pr[i].elapsed_ms for pr in progs for i in R)
        out = {"workload": "config[2] on this one GPU: %d independent 1080p pairs (%d distinct frames), %d stream(s) x batches of %d pairs per "
                           "launch, one step" % (len(mine), distinct, nctx, B),
               "value": round(live / dt / 1e6, 2), "value_nominal": round(nominal / dt / 1e6, 2), "unit": "Mpixel*iters/s",
               "ms_per_step": round(dt * 1e3, 2), "executed_pixel_iters": round(live),
               "sclk_mhz_observed": {"dense_tile_kernel": clock_mhz(progs, R, 0), "k_pass": clock_mhz(progs, R, 1)},
               "sweep_kernel_ms_summed_over_streams": round(kern_ms, 1),
               "note": "`python bench.py --gpus N` (N > 1) shards exactly this job over N ranks: divide its value by this one"}
        out.update(activity(progs, R, dt, dt * 1e3))          # valu_frac against wall time (streams overlap)
        return out
    except Exception as e:                                     # noqa: BLE001 -- reported, never fatal
        return {"error": str(e)[-300:]}
    finally:
        for p in pyrs:
            try:
                p.clear()
            except Exception:
                pass
        for c in ctxs:
            try:
                c.close()
            except Exception:
                pass


def load_poisson_pmc(path=None):
    """PMC traffic of the Poisson solver's kernels per system and PCG iteration, from the committed profile of the 4-frame
    batch (profiles/poisson_traffic_latest.json, written by tools/prof_pmc.sh + tools/pmc_summary.py); None if absent"""
    try:
        d = json.load(open(path or os.path.join(ROOT, "profiles", "poisson_traffic_latest.json")))
        per = d.get("per_kernel_bytes_per_launch", {})
        nsys = float(d.get("systems_per_launch", 8))
        dominant = {name: per[key] / nsys for name, key in (("k_mgb_update", "k_mgb_update"), ("k_mgb_restrict<true, true>", "void k_mgb_restrict<true, true>"))
                    if per.get(key)}
        return {"bytes_per_system_iteration": float(d["bytes_per_system_iteration"]), "source": d["source"],
                "dominant_bytes_per_system_launch": dominant}
    except Exception:
        return None


def sweep_source_hash():
    """fingerprint of the sources the sweep kernels are compiled from (tools/pmc_summary.py stamps every entry of
    profiles/traffic_latest.json with it when the entry is merged)"""
    import hashlib
    h = hashlib.sha256()
    for f in ("vm_sweep_kernels.hip", "vm_morph_common.h", "vm_internal.h"):
        h.update(open(os.path.join(ROOT, "videomorphing_amd", "csrc", f), "rb").read())
    return h.hexdigest()


def load_pmc(config, pairs_per_launch, path=None):
    """HBM bytes per launch of the sweep kernels from the committed PMC profile of THIS workload
    shape (config, pairs per launch); counters need rocprofv3, so they are never of this run.
    No matching entry: no PMC figures (a figure taken at another batch size would be wrong).
    Returns (bytes per kernel, launches per kernel, source text, SQ counters per kernel, stale): stale is True when the
    sweep kernels' sources have changed since the entry was profiled (or the entry carries no fingerprint) -- the one
    roofline input the driver cannot re-derive must not outlive the kernels it describes unnoticed."""
    tp = path or os.path.join(ROOT, "profiles", "traffic_latest.json")
    try:
        tj = json.load(open(tp))
    except Exception:
        return {}, {}, None, {}, None
    for e in tj.get("entries", []):
        if e.get("config") == config and e.get("pairs_per_launch") == pairs_per_launch:
            try:
                stale = e.get("sweep_source_sha256") != sweep_source_hash()
            except Exception:
                stale = True
            return e.get("per_kernel", {}) or {}, e.get("per_kernel_launches", {}) or {}, \
                "%s[config %d, %d pair(s) per launch]: %s" % (
                    os.path.relpath(tp, ROOT), config, pairs_per_launch, e.get("source", "")[:200]), e.get("sq_per_kernel", {}) or {}, stale
    return {}, {}, None, {}, None


def sq_measured(sq, prefix):
    """SQ counters of the committed profile of this workload shape for the kernels of one schedule
    (template variants weighted by their launches): how busy the vector ALUs were, MEASURED --
    valu_frac above is a flop count divided by a peak."""
    ks = [k for k in sq if k.startswith(prefix) and sq[k].get("SQ_WAVE_CYCLES")]
    if not ks:
        return None
    tot = lambda c: sum(sq[k].get(c, 0.0) * sq[k].get("calls", 1.0) for k in ks)
    wc, grbm = tot("SQ_WAVE_CYCLES"), tot("GRBM_GUI_ACTIVE")
    out = {"valu_active_of_wave_cycles": round(tot("SQ_ACTIVE_INST_VALU") / wc, 4),
           "wait_any_of_wave_cycles": round(tot("SQ_WAIT_ANY") / wc, 4),
           "wait_inst_any_of_wave_cycles": round(tot("SQ_WAIT_INST_ANY") / wc, 4),
           "valu_insts_per_wave": round(tot("SQ_INSTS_VALU") / max(tot("SQ_WAVES"), 1.0), 1)}
    if grbm > 0:
        # 1024 SIMDs issue one wave64 VALU instruction per 4 cycles; GRBM_GUI_ACTIVE is summed over the 8 XCDs
        out["valu_issue_slots_used"] = round(tot("SQ_INSTS_VALU") * 4.0 / (1024.0 * grbm / 8.0), 4)
    if tot("SQ_LDS_IDX_ACTIVE") > 0:
        out["lds_bank_conflict_of_lds_active"] = round(tot("SQ_LDS_BANK_CONFLICT") / tot("SQ_LDS_IDX_ACTIVE"), 4)
    return out


def pmc_bytes(pmc_k, pmc_n, prefix):
    """launch-weighted mean of the PMC bytes per launch over the kernels whose name starts with prefix"""
    ks = [k for k in pmc_k if k.startswith(prefix)]
    if not ks:
        return None
    n = sum(pmc_n.get(k, 1) for k in ks)
    return sum(pmc_k[k] * pmc_n.get(k, 1) for k in ks) / max(n, 1)


def report(args, config, world, w, h, nlev, blk, capi, B, nctx, FIXED, sizes, progs, step_ms, el_max, pix_total, cpu,
           distinct_frames, pairs_this_rank, pix_live_total, frame_ids=None):
    R = range(nlev - 1)
    nsolve = max(len(progs), 1)
    kern_ms = sum(pr[i].elapsed_ms for pr in progs for i in R)
    launches = sum(pr[i].launches for pr in progs for i in R)
    # ---- algorithmic bytes: 100 B per pixel-visit; NOMINAL counts every visit of
    # every executed iteration, EXECUTED only the tile visits the improving mask did not skip
    alg_nominal = sum(pr[i].iters * tile_visits(*sizes[i]) * ALG_BYTES_PER_VISIT for pr in progs for i in R)
    pixel_visits = sum(pr[i].iters * tile_visits(*sizes[i]) for pr in progs for i in R)
    active_tiles = sum(pr[i].active_tiles for pr in progs for i in R)
    line_searches = sum(pr[i].candidates for pr in progs for i in R)
    commits = sum(pr[i].commits for pr in progs for i in R)
    evals = sum(pr[i].evaluations for pr in progs for i in R)
    alg_executed = active_tiles * 64 * 16 * ALG_BYTES_PER_VISIT
    achieved = alg_nominal / (kern_ms * 1e-3) / 1e9 if kern_ms > 0 else 0.0
    # ---- HBM traffic per launch from the PMC passes of the committed profile of this workload
    # shape (not of this run: counters need rocprofv3)
    pmc_k, pmc_n, traffic_src, sq_k, traffic_stale = load_pmc(config, B)
    # ---- per kernel: launches, average duration (HIP events around each batch of launches on
    # the context's stream), algorithmic bytes per launch, nominal and real fraction of HBM peak
    per_kernel = []
    for k in range(NSCHED):
        ms = sum(pr[i].sched_ms[k] for pr in progs for i in R)
        n = sum(pr[i].sched_launches[k] for pr in progs for i in R)
        if n == 0:
            continue
        # one TILE or PASS launch = one pass over the level (a quarter of an iteration's visits) of
        # every pair of the batch; one STEP launch = one phase of one pass (a sixteenth); a SPARSE
        # launch covers a whole batch of iterations: its nominal bytes are those of the iterations
        # it executed (the level's executed iterations minus what the other schedules account for)
        nbytes = 0.0
        for pr_i, pr in enumerate(progs):
            for i in R:
                if pr[i].sched_launches[k]:
                    # launches are recorded once per batch (first pair); the batch's other pairs add their visits
                    if k == 3:
                        others = sum(pr[i].sched_launches[j] / SCHED_LAUNCHES_PER_ITER[j] for j in range(NSCHED) if j != 3)
                        nbytes += max(pr[i].iters_live - others, 0.0) * tile_visits(*sizes[i]) * ALG_BYTES_PER_VISIT * B
                    else:
                        nbytes += pr[i].sched_launches[k] * tile_visits(*sizes[i]) / SCHED_LAUNCHES_PER_ITER[k] * ALG_BYTES_PER_VISIT * B
        avg_us = ms * 1e3 / n
        ent = {"kernel": SCHED[k], "launches": n, "avg_us": round(avg_us, 2), "share_of_sweep_time": round(ms / max(kern_ms, 1e-9), 3),
               "alg_bytes_per_launch": round(nbytes / n), "nominal_GBs": round(nbytes / n / (avg_us * 1e-6) / 1e9, 2),
               "nominal_frac": round(nbytes / n / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 5)}
        pb = pmc_bytes(pmc_k, pmc_n, SCHED_PMC[k])
        if pb is not None:
            ent["pmc_bytes_per_launch"] = round(pb)
            ent["real_GBs"] = round(pb / (avg_us * 1e-6) / 1e9, 2)
            ent["real_frac"] = round(pb / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 5)
            ent["traffic_over_algorithmic"] = round(pb / max(nbytes / n, 1.0), 2)
        sqm = sq_measured(sq_k, SCHED_PMC[k])
        if sqm is not None:
            ent["sq_measured"] = sqm
        per_kernel.append(ent)
    avg_launch_us = kern_ms * 1e3 / max(launches, 1)
    # the kernel the job spends most of its sweep time in: the roofline line is ITS
    dom = max(per_kernel, key=lambda e: e["share_of_sweep_time"]) if per_kernel else None
    pmc_total = sum(e.get("pmc_bytes_per_launch", 0) * e["launches"] for e in per_kernel)
    hbm_real_frac = (pmc_total / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if (pmc_total and kern_ms > 0) else None
    steps = args.steps
    out = {
        "metric": "Mpixel*iters/s (halfway optimizer, 1080p pair, 6-level pyramid, 500 iters/level)" if config != 3 else
                  "Mpixel*iters/s (halfway optimizer, 3840x2160 pair, 7-level pyramid, 500 iters/level)",
        # EXECUTED pixel*iters / wall time: the reference's own progress unit (`_current_iter += W*H` per sweep that
        # runs, morph.cu:1389) -- sweeps up to and including each level's first without an accepted move
        "value": round(pix_live_total / el_max / 1e6, 2),
        "unit": "Mpixel*iters/s",
        "n_gpus": world, "steps": steps, "warmup": args.warmup,
        "ms_per_step": round(el_max / steps * 1e3, 2),
        "higher_is_better": True, "scaling": "strong" if config == 2 else "weak", "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic" if config != 2 else "synthetic (%d distinct frames on rank 0: every pair its own frame)" % distinct_frames,
        "config": {"workload": workload_name(config, w, h, nlev, blk, B, args, world, pairs_this_rank),
                   "math_mode": "fast" if blk.math_mode == capi.MATH_FAST else "exact",
                   "semantics": ("every level gets max_iter = 500 sweeps ('500 iters/level'); a level that stops improving needs no more "
                                 "of them -- the remaining sweeps are provable no-ops the device skips -- so `value` counts the EXECUTED "
                                 "sweeps only (up to and including each level's first without an accepted move: what the reference's loop "
                                 "runs, morph.cu:1378-1390); value_nominal credits all 500 per level and is NOT a throughput") if FIXED
                                else "reference: a level stops when no pixel improved",
                   "iters_per_level_fine_to_coarse": [progs[0][i].iters for i in R],
                   "iters_executed_per_level_fine_to_coarse": [progs[0][i].iters_live for i in R],
                   "pairs_in_flight_per_gpu": nctx, "pairs_per_launch": B,
                   "parallelism": "independent frame pairs, %d rank(s), 1 RCCL broadcast + 1 all-gather of the report" % world},
        "executed_pixel_iters": round(pix_live_total),
        # max_iter sweeps credited for every level whether they ran or not (rounds 1-3 quoted this one)
        "value_nominal": round(pix_total / el_max / 1e6, 2),
        # what the chip did per second of wall time (rank 0's share x ranks), whatever the units credited: energy evaluations
        # (each 2 bilinear taps + 25 SSIM terms), line searches, and SURVEY 8(d)'s VALU fraction of the sweep kernels
        "evals_per_s": round(evals * world / el_max), "line_searches_per_s": round(line_searches * world / el_max),
        "valu_frac": round(evals * FLOP_PER_EVAL / (kern_ms * 1e-3) / VALU_PEAK_FLOPS, 5) if kern_ms > 0 else None,
        # the shader clock actually held INSIDE the two chain-bound kernels (in-kernel probe: s_memtime / s_memrealtime of
        # their first workgroup, every launch of the timed region); the VALU peak above assumes 2400 MHz
        "sclk_mhz_observed": {"k_pass": clock_mhz(progs, R, 1), "dense_tile_kernel": clock_mhz(progs, R, 0), "assumed_by_valu_peak": 2400},
        "roofline": {"bound": "hbm",
                     # the dominant sweep kernel (largest share of sweep time): ALGORITHMIC bytes of one
                     # launch (100 B per pixel-visit x the visits one launch covers) / its
                     # average duration (HIP events on the context's stream)
                     "kernel": dom["kernel"] if dom else None,
                     "achieved": dom["nominal_GBs"] if dom else None,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": dom["nominal_frac"] if dom else None,
                     "traffic": dom.get("pmc_bytes_per_launch") if dom else None,
                     "traffic_source": traffic_src,
                     "traffic_stale": traffic_stale,     # True: the sweep kernels' sources changed since that profile was taken
                     "launch_us": dom["avg_us"] if dom else None,
                     "alg_bytes_per_launch": dom["alg_bytes_per_launch"] if dom else None,
                     "share_of_sweep_time": dom["share_of_sweep_time"] if dom else None,
                     # SURVEY 8(d)'s formula on the EXECUTED rate: value x 282.7 B per pixel*iter / 8 TB/s.  Algorithmic
                     # bytes INCLUDING the tile visits the improving mask skips (2.827 visits per pixel and sweep are
                     # counted whether or not a tile has a candidate): not a bandwidth statement -- hbm_real_frac is
                     "survey_formula_executed": round(pix_live_total / el_max * ALG_BYTES_PER_VISIT * 2.827 / 1e9 / HBM_PEAK_GBS, 5),
                     # the same formula over every CREDITED sweep (skipped no-op sweeps included) / HIP-event time:
                     # bytes that were never moved (it exceeds 1 on batched jobs); kept only to read older rounds' lines
                     "credited_not_moved": {"GBs": round(achieved, 2), "frac_of_peak": round(achieved / HBM_PEAK_GBS, 5)},
                     "achieved_executed": round(alg_executed / (kern_ms * 1e-3) / 1e9, 2) if kern_ms > 0 else None,
                     "frac_executed": round(alg_executed / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if kern_ms > 0 else None,
                     "hbm_real_frac": round(hbm_real_frac, 5) if hbm_real_frac is not None else None,
                     "avg_launch_us": round(avg_launch_us, 2), "launches": launches,
                     "alg_bytes_per_pixel_visit": ALG_BYTES_PER_VISIT,
                     "valu_frac": round(evals * FLOP_PER_EVAL / (kern_ms * 1e-3) / VALU_PEAK_FLOPS, 5) if kern_ms > 0 else None,
                     "flop_per_evaluation": FLOP_PER_EVAL,
                     # MEASURED (SQ counters of the committed profile of this workload shape) for the dominant kernel
                     "valu_busy_measured": dom.get("sq_measured") if dom else None,
                     "active_pixel_ratio": round(line_searches / max(pixel_visits, 1), 6),
                     "per_kernel": per_kernel},
        "cpu_baseline": cpu,
        "activity_per_solve": {"active_tile_visits": round(active_tiles / nsolve), "line_searches": round(line_searches / nsolve),
                               "energy_evaluations": round(evals / nsolve), "commits": round(commits / nsolve),
                               "pixel_visits": round(pixel_visits / nsolve)},
    }
    if step_ms:
        ms = sorted(step_ms)
        out["step_ms"] = {"each": [round(x, 2) for x in step_ms], "min": round(ms[0], 2), "median": round(statistics.median(ms), 2),
                          "max": round(ms[-1], 2),
                          "note": "every step is a different frame of the synthetic video; whether the finest level converges or "
                                  "keeps exchanging rounding-level moves differs per frame" if config != 2 else "every step re-solves the rank's pairs"}
        # executed units of each step / that step's time: the median step instead of the mean
        per = max(len(progs) // max(len(step_ms), 1), 1)
        rates = []
        for k, t_ms in enumerate(step_ms):
            live = sum(float(pr[i].iters_live) * sizes[i][0] * sizes[i][1] for pr in progs[k * per:(k + 1) * per] for i in R)
            rates.append(live * world / (t_ms * 1e-3) / 1e6)
        out["value_median_step"] = round(statistics.median(rates), 2)
        # a step whose finest level ran all of its sweeps (two or three border pixels trading rounding-level moves: about one
        # solve in four, under any arithmetic) executes ~5x the units of one whose finest level converged, in ~1.4x the time:
        # the two kinds of step, apart
        if config != 2 and per == 1:
            cyc = [int(progs[k][0].iters_live >= progs[k][0].iters and progs[k][0].iters > 1) for k in range(len(step_ms))]
            for name, sel in (("steps_finest_level_cycling", 1), ("steps_finest_level_converging", 0)):
                ks = [k for k in range(len(step_ms)) if cyc[k] == sel]
                if ks:
                    out[name] = {"count": len(ks), "ms_mean": round(sum(step_ms[k] for k in ks) / len(ks), 2),
                                 "mpix_iters_per_s": round(sum(rates[k] for k in ks) / len(ks), 2),
                                 "executed_mpix_iters_mean": round(sum(rates[k] * step_ms[k] * 1e-3 for k in ks) / len(ks), 1)}
            # which frames they are: `value` moves with the NUMBER of cycling frames (a cycling step executes ~5x the units
            # in ~1.4x the time), so a round that changes that number cannot move the headline unnoticed; the two
            # comparable figures are ms_converging_steps and ms_cycling_steps
            if frame_ids is not None and len(frame_ids) == len(step_ms):
                out["config"]["frame_ids"] = list(frame_ids)
                out["config"]["cycling_frame_ids"] = [frame_ids[k] for k in range(len(step_ms)) if cyc[k]]
            conv = [step_ms[k] for k in range(len(step_ms)) if not cyc[k]]
            cycl = [step_ms[k] for k in range(len(step_ms)) if cyc[k]]
            out["ms_converging_steps"] = round(statistics.median(conv), 2) if conv else None
            out["ms_cycling_steps"] = round(statistics.median(cycl), 2) if cycl else None
        out["step_executed_mpix_iters"] = [round(sum(float(pr[i].iters_live) * sizes[i][0] * sizes[i][1] for pr in progs[k * per:(k + 1) * per]
                                                     for i in R) / 1e6, 2) for k in range(len(step_ms))]
    return out


def workload_name(config, w, h, nlev, blk, B, args, world, pairs_this_rank):
    base = "%dx%d frame pair, %d-level pyramid (start_res %d), max_iter %d/level, drop %g" % (
        w, h, nlev, blk.start_res, int(blk.max_iter), blk.max_iter_drop_factor)
    if config == 2:
        return ("config[2]: %d independent %s; sharded over %d rank(s) (rank 0: %d pairs), solved per rank in batches of <= %d "
                "pairs per launch; one step = the whole job" % (args.pairs, base, world, pairs_this_rank, B))
    return "config[%d]: %s, %s per step per GPU" % (config, base, "one pair" if B == 1 else "a batch of %d independent pairs" % B)


def run_extras(args, np, capi, morph, synth, L, blk, ctx, p, w, h, nlev, FIXED, B, solve, solve_group, local_rank=0, frames=None):
    """context numbers beside the headline (rank 0, one GPU): the other stopping rule, the other
    arithmetic, batched throughput, compositor stages, config[3] and config[4] in one step each.
    --extras a,b,... (development) runs only the named ones."""
    only = set(x for x in args.extras.split(",") if x)
    want = lambda name: not only or name in only
    saved_kp = capi.KernParams()      # extras that bring their own Parameters put these back
    capi.check(L.vm_get_params(ctx._h, C.byref(saved_kp)))
    extras = {}
    R = range(nlev - 1)
    sz = [(p[el].width, p[el].height) for el in range(1, nlev)]
    executed = lambda prs: sum(float(q[i].iters_live) * sz[i][0] * sz[i][1] for q in prs for i in R)
    if want("semantics"):
        ctx.sync(); t1 = time.perf_counter(); pr = solve(p, fixed=1 - FIXED); ctx.sync(); dt = time.perf_counter() - t1
        extras["%s_semantics" % ("reference" if FIXED else "fixed")] = {
            "mpix_iters_per_s": round(executed([pr]) / dt / 1e6, 2),
            "ms_per_solve": round(dt * 1e3, 2),
            "iters_per_level_fine_to_coarse": [pr[i].iters for i in R]}
    if want("math"):
        other = capi.MATH_EXACT if blk.math_mode == capi.MATH_FAST else capi.MATH_FAST
        ctx.set_math_mode(other)
        ctx.sync(); t1 = time.perf_counter(); pr = solve(p); ctx.sync(); dt = time.perf_counter() - t1
        extras["%s_math" % ("exact" if other == capi.MATH_EXACT else "fast")] = {
            "mpix_iters_per_s": round(executed([pr]) / dt / 1e6, 2), "ms_per_solve": round(dt * 1e3, 2),
            "iters_executed_per_level_fine_to_coarse": [pr[i].iters_live for i in R]}
        ctx.set_math_mode(blk.math_mode)
    if w * h > 1920 * 1080:
        return extras
    # batched throughput: B independent pairs relaxed by the same launches (the per-GPU workload
    # of config[2]); 4 distinct frames reused cyclically
    base_frames = [synth.make_pair(w, h, frame=1000 + k) for k in range(4)]
    if B == 1 and want("batched"):
        bt = {}
        for nb in (8, 32):
            group = []
            for k in range(nb):
                q = morph.Pyramid(ctx)
                q.build(base_frames[k % 4][0], base_frames[k % 4][1], blk.start_res, nlevels=nlev)
                group.append(q)
            solve_group(group)                                    # warm-up
            ctx.sync(); t1 = time.perf_counter(); pr = solve_group(group); ctx.sync()
            dt = time.perf_counter() - t1
            bt["pairs_%d" % nb] = {
                "mpix_iters_per_s": round(executed(pr) / dt / 1e6, 1),
                "nominal_mpix_iters_per_s": round(sum(q2[i].pixel_iters for q2 in pr for i in R) / dt / 1e6, 1),
                "ms_per_batch": round(dt * 1e3, 1)}
            del group
        extras["batched_throughput"] = bt
    # the temporally coupled path: a 5-frame 1080p video pair with analytic
    # flows, every frame tied to its solved neighbour (middle page, then both chains, two pages
    # per launch); the device-side flow pyramid included, lumas uploaded per page
    if want("temporal"):
        try:
            d = 5
            levels, ft = synth.video_levels(w, h, d, blk.start_res)
            vid = morph.VideoPyramid(ctx)
            vid.build_levels(levels, ft, d)
            pages = synth.page_frames(levels, ft)
            vf = [synth.make_video_pair(w, h, t) for t in range(d)]
            vp = [synth.build_pyramid(a, b2, len(levels)) for a, b2 in vf]
            for l in range(len(levels) - 1):
                for t in range(levels[l][2]):
                    vid.upload_luma(l, t, *vp[pages[l][t]][l])
            flows = synth.constant_flows(w, h, d)
            vid.build_flows(*flows)                         # warm-up (scratch planes are allocated on first use)
            ctx.sync(); t1 = time.perf_counter()
            vid.build_flows(*flows)
            ctx.sync(); t_flow = time.perf_counter() - t1
            prm = morph.Parameters()
            prm.max_iter, prm.max_iter_drop_factor, prm.start_res = int(blk.max_iter), blk.max_iter_drop_factor, blk.start_res
            vm = morph.VideoMorph(prm, vid, fixed_work=bool(FIXED))
            vm.calculate_halfway_parametrization()          # warm-up (workspaces)
            ctx.sync(); t1 = time.perf_counter()
            vm.calculate_halfway_parametrization()
            ctx.sync(); dt = time.perf_counter() - t1
            units = sum(l[0] * l[1] * pr["iters_live"] for (lv, t), pr in vm.progress.items() for l in [levels[lv]])
            nominal = sum(l[0] * l[1] * pr["iters"] for (lv, t), pr in vm.progress.items() for l in [levels[lv]])
            extras["temporal_video_%d_frames" % d] = {"mpix_iters_per_s": round(units / dt / 1e6, 1), "nominal_mpix_iters_per_s": round(nominal / dt / 1e6, 1),
                                                      "ms_per_video": round(dt * 1e3, 1),
                                                      "flow_pyramid_ms": round(t_flow * 1e3, 1),
                                                      "depth_per_level": [l[2] for l in levels]}
            # ... and on to the screen (CMatchingThread::update_result for a video, then the compositor):
            # per frame of the video its full-resolution field straight into a device-resident frame
            # (vm_frame_set_v_from_video), Poisson extension of both sides (one batch), 9 rendered in-between
            # frames; canvases uploaded once per frame (PCIe included)
            exv = int(0.1 * max(w, h))
            rv0, rv1 = synth.make_rgb_pair(w, h)
            ev0, ev1 = morph.make_extended(rv0, exv), morph.make_extended(rv1, exv)
            frv = morph.Frame(ctx, w, h, exv)
            frv.upload(ev0, ev1, None, None)
            frv.set_v_from_video(vid, 0, 0)
            frv.poisson_extend_both(tol=POISSON_TOL)          # workspaces
            ctx.sync(); t1 = time.perf_counter()
            for fidx in range(d):
                frv.upload(ev0, ev1, None, None)
                frv.set_v_from_video(vid, 0, fidx)
                frv.poisson_extend_both(tol=POISSON_TOL)
                for k in range(1, 10):
                    frv.render_halfway_dev(0.1 * k, 0.1 * k, 1)
            ctx.sync(); dtv = time.perf_counter() - t1
            frv.close()
            extras["video_pipeline_%d_frames" % d] = {"compositor_ms_per_video_frame": round(dtv * 1e3 / d, 1),
                                                      "rendered_frames_per_s": round(d * 9 / dtv, 1),
                                                      "solve_plus_compositor_ms_per_video": round((dt + dtv) * 1e3, 1)}
            del vid
        except capi.VmError as e:
            extras["temporal_video_5_frames"] = {"error": str(e)[-160:]}
        finally:
            ctx.set_params(saved_kp)
    # the synchronisation stage that precedes the morph in the reference's app (CSyncThread +
    # render_resample_image, SURVEY 8(f) "(later)"): a 1080p x 60-frame pair, 24 constraints across
    # frames, the reference's iteration schedule (max_iter * 10 at the coarsest level, halved per
    # level).  HBM-bound: 124 algorithmic bytes per voxel and CG iteration.
    if want("sync"):
        try:
            extras["sync_stage_1080p_x60"] = sync_stage_extra(np, morph, ctx, w, h, 60, blk)
        except capi.VmError as e:
            extras["sync_stage_1080p_x60"] = {"error": str(e)[-160:]}
        finally:
            ctx.set_params(saved_kp)        # the sync stage runs with its own w_ui / w_tps
    # compositor: frames/s of render_halfway with device-resident inputs (Metric 2, render only)
    ex = int(0.1 * max(w, h))
    if not any(want(x) for x in ("render", "poisson", "qpath", "pipeline8", "pipeline30", "config3")):
        return extras
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    fr = morph.Frame(ctx, w, h, ex)
    e0, e1 = morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex)
    fr.upload(e0, e1, None, None)
    fr.set_v_from_level(p, 1)
    render_ms = None
    if want("render") or want("pipeline30"):
        fr.render_halfway_dev(0.5, 0.5, 1)
        ms = [fr.render_halfway_dev(0.5, 0.1 * k, 1) for k in range(1, 10)]
        render_ms = sum(ms) / len(ms)
        extras["render_frames_per_s"] = round(1000.0 / render_ms, 1)
        # ... and with a quadratic path in the frame (the renderer then follows u as well: twice the dependent taps); the
        # figure above is the reference app's state -- its quadratic-path stage is commented out, `_qpath` stays zero
        qp = (0.25 * synth.displacement(w, h)).astype(np.float32)
        fr.upload(None, None, None, qp)
        fr.render_halfway_dev(0.5, 0.5, 1)
        ms = [fr.render_halfway_dev(0.5, 0.1 * k, 1) for k in range(1, 10)]
        extras["render_frames_per_s_with_quadratic_path"] = round(1000.0 / (sum(ms) / len(ms)), 1)
        fr.upload(None, None, None, None)
    # Poisson boundary extension of both sides of that frame (config[4]'s other stage): the two sides as one batch
    # (vm_poisson_extend_frames), and -- for the record of what batching buys -- one side at a time
    if want("poisson"):
        pe = {}
        fr.poisson_extend_both(tol=1e-3)      # the workspaces are allocated on first use: not timed
        # timed ONLY at tolerances the full-size oracle fixtures verify (max |colour difference| <= 1 against the oracle's CG
        # at 1e-9 on this very canvas: tests/test_gpu_fullsize_compositor.py); SURVEY 8(d)'s own figure is 1e-6
        for tol in POISSON_TIMED_TOLS:
            fr.upload(e0, e1, None, None)
            (i1, _), (i2, _), ms_both = fr.poisson_extend_both(tol=tol)
            pe["tol_%g" % tol] = {"ms_per_frame": round(ms_both, 2), "cg_iterations": [i1, i2]}
        fr.upload(e0, e1, None, None)
        r1, r2 = fr.poisson_extend(1, tol=POISSON_TOL), fr.poisson_extend(2, tol=POISSON_TOL)
        pe["tol_%g_one_side_at_a_time" % POISSON_TOL] = {"ms_per_frame": round(r1[2] + r2[2], 2), "cg_iterations": [r1[0], r2[0]]}
        # four frames per batch (eight systems per launch): the shape the config[4] pipeline runs
        frs4 = [fr] + [morph.Frame(ctx, w, h, ex) for _ in range(3)]
        dom = None
        try:
            for tol in POISSON_TIMED_TOLS:
                best4 = None
                for rep in range(2):
                    for f4 in frs4:
                        f4.upload(e0, e1, None, None)
                        if f4 is not fr:
                            f4.set_v_from_level(p, 1)
                    res4, ms4 = morph.poisson_extend_frames(frs4, tol=tol)
                    best4 = ms4 if best4 is None else min(best4, ms4)
                pe["tol_%g_four_frames_per_batch" % tol] = {"ms_per_frame": round(best4 / 4, 2), "cg_iterations": [s_[0] for r in res4 for s_ in r]}
            # the dominant kernel of the solve, measured live (HIP events around every k_mgb_update launch on the stream it
            # is launched on: vm_dbg_poisson_profile), one more 4-frame batch, not among the timed ones
            for f4 in frs4:
                f4.upload(e0, e1, None, None)
                if f4 is not fr:
                    f4.set_v_from_level(p, 1)
            ctx.poisson_profile(True)
            morph.poisson_extend_frames(frs4, tol=POISSON_TOL)
            dom = ctx.poisson_profile(False)
        finally:
            for f4 in frs4[1:]:
                f4.close()
        # roofline of the solve: algorithmic bytes = unknowns x PCG iterations x 178 B (level 0: update + restriction
        # in one kernel 76, prolongation 28, direction / operator 49; coarse levels ~25, their second sweep from level 2 down < 2)
        # over the HIP-event time of the batch (classification, fill, hierarchy set-up and paste included in the time, not in
        # the bytes: with fewer, stronger iterations this fraction FALLS while the solve gets faster -- the dominant kernel's
        # fraction below is the bandwidth statement)
        unknowns = (w + 2 * ex) * (h + 2 * ex) - (w - 2) * (h - 2)         # outside pixels + the one-pixel ring inside
        key = "tol_%g" % POISSON_TOL
        its = pe[key]["cg_iterations"]
        alg = unknowns * sum(its) * POISSON_ALG_BYTES
        gbs = alg / (pe[key]["ms_per_frame"] * 1e-3) / 1e9
        its4 = pe[key + "_four_frames_per_batch"]["cg_iterations"]
        gbs4 = unknowns * sum(its4) * POISSON_ALG_BYTES_FUSED / (4 * pe[key + "_four_frames_per_batch"]["ms_per_frame"] * 1e-3) / 1e9
        pmc = load_poisson_pmc()
        # the launch that carries the PCG update, average of a 4-frame batch, HIP events in this run: in a batch of eight systems the
        # level-0 restriction with the update fused in (reads p, q, x, r and the operator byte, writes x, r and the coarse right-hand
        # side = 76 B per unknown of every active system); k_mgb_update by itself (73 B) if the library did not fuse.
        # profiles/r06_poisson4_kernel_stats.csv holds rocprofv3's average of the same kernel
        fused = bool(dom) and dom[1] > 0 and dom[3] == dom[1]
        dk_name, dk_bytes = ("k_mgb_restrict<true, true>", 76.0) if fused else ("k_mgb_update", 73.0)
        pe["roofline"] = {"bound": "hbm", "kernel": "multigrid-PCG solve of both sides of one frame as one batch (12 launches per iteration; the level-0 "
                                                     "kernels k_mgb_restrict<true, true> (with the PCG update) / k_mgb_dirspmv / k_mgb_prolong: profiles/r06_compositor_*)",
                          "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                          "four_frames_per_batch": {"achieved": round(gbs4, 1), "frac": round(gbs4 / HBM_PEAK_GBS, 4),
                                                    "alg_bytes_per_unknown_iteration": POISSON_ALG_BYTES_FUSED,
                                                    "kernel": "the same solve, four frames = eight systems per batch"},
                          "dominant_kernel": dom and dom[1] > 0 and {
                              "kernel": dk_name, "launches": dom[1], "launch_us": round(dom[0] / dom[1], 2),
                              "alg_bytes_per_unknown": dk_bytes,
                              "alg_bytes_per_launch": round(dom[2] / dom[1] * unknowns * dk_bytes),
                              "achieved": round(dom[2] * unknowns * dk_bytes / (dom[0] * 1e-6) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round(dom[2] * unknowns * dk_bytes / (dom[0] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                              "traffic": pmc and pmc.get("dominant_bytes_per_system_launch", {}).get(dk_name) and
                              round(pmc["dominant_bytes_per_system_launch"][dk_name] * dom[2] / dom[1])},
                          "traffic": round(pmc["bytes_per_system_iteration"] * sum(its)) if (pmc and (w, h, ex) == (1920, 1080, 192)) else None,
                          "traffic_source": pmc and pmc["source"],
                          "alg_bytes_per_unknown_iteration": POISSON_ALG_BYTES, "unknowns_per_side": unknowns, "tol": POISSON_TOL}
        extras["poisson_extend_1080p_ex%d" % ex] = pe
    # quadratic motion path of that frame (QuadraticPath.cpp), SURVEY 8(f) rank 4
    if want("qpath"):
        fr.set_v_from_level(p, 1)
        try:
            fr.quadratic_path(tol=1e-3)      # the workspace is allocated on first use: not timed
            qp = fr.quadratic_path(tol=1e-4)     # float32 attains 1e-4 on a solved field; 2e-3 px of the oracle at full size: tests/test_gpu_fullsize_compositor.py
            extras["quadratic_path_1080p"] = {"ms_per_frame": round(qp[2], 2), "pcg_iterations": qp[0], "tol": 1e-4,
                                              "residual": float("%.3g" % qp[1])}
        except capi.VmError as e:        # e.g. a folded v: the blend of the Jacobians is 0/0 there
            extras["quadratic_path_1080p"] = {"error": str(e)[-120:]}
    # config[4]'s whole pipeline on one GPU: 8 frame pairs solved as a batch (reference
    # semantics), then per frame v upscale -> Poisson extension of both sides -> 9 rendered
    # in-between frames; canvases uploaded once per frame (PCIe included)
    if B == 1 and want("pipeline8"):
        group = []
        for k in range(8):
            q = morph.Pyramid(ctx)
            q.build(base_frames[k % 4][0], base_frames[k % 4][1], blk.start_res, nlevels=nlev)
            group.append(q)
        ctx.sync(); t1 = time.perf_counter()
        morph.solve_batch(group, blk.max_iter, blk.max_iter_drop_factor, fixed_work=False)
        t_solve = time.perf_counter() - t1
        for q in group:
            fr.upload(e0, e1, None, None)
            fr.set_v_from_level(q, 1)
            fr.poisson_extend_both(tol=POISSON_TOL)
            for k in range(1, 10):
                fr.render_halfway_dev(0.1 * k, 0.1 * k, 1)
        ctx.sync(); dt = time.perf_counter() - t1
        extras["pipeline_config4_8_pairs"] = {"ms_per_pair": round(dt * 1e3 / 8, 1), "solve_ms_per_pair": round(t_solve * 1e3 / 8, 1),
                                              "rendered_frames_per_s": round(8 * 9 / dt, 1)}
        del group
    fr.close()
    # config[4] as BASELINE.json states it, on this one GPU: THIRTY 1080p frame pairs with 8 point constraints each and
    # BCOND_BORDER, solved in batches (reference semantics); then the compositor over all thirty frames: canvases
    # uploaded once per frame (PCIe included), v upscaled on the device, Poisson extension of both sides of FOUR frames
    # per batch (8 systems per launch), 9 rendered in-between frames per pair
    if B == 1 and want("pipeline30"):
        try:
            extras["pipeline_config4_30_frames"] = pipeline30(np, capi, morph, synth, ctx, blk, w, h, nlev, rgb0, rgb1, ex, render_ms, local_rank, frames, POISSON_TOL)
        except capi.VmError as e:
            extras["pipeline_config4_30_frames"] = {"error": str(e)[-200:]}
        finally:
            ctx.set_params(saved_kp)
    # config[3] (3840x2160, 7 levels) in one step, for the driver's record (`--config 3` runs it as the headline)
    if B == 1 and want("config3"):
        try:
            w3, h3 = CONFIG_SIZE[3]
            nl3 = synth.num_levels(w3, h3, blk.start_res)
            i0, i1 = synth.make_pair(w3, h3, frame=0)
            q = morph.Pyramid(ctx)
            q.build(i0, i1, blk.start_res, nlevels=nl3)
            sz3 = [(q[el].width, q[el].height) for el in range(1, nl3)]
            best = None
            for rep in range(2):                         # the first solve allocates the schedule workspaces
                prog = (capi.Progress * (nl3 - 1))()
                ctx.sync(); t1 = time.perf_counter()
                capi.check(L.vm_solve(q._h, blk.max_iter, blk.max_iter_drop_factor, None, 0, None, FIXED, prog))
                ctx.sync(); best = time.perf_counter() - t1
            live3 = sum(float(prog[i].iters_live) * sz3[i][0] * sz3[i][1] for i in range(nl3 - 1))
            extras["config3_4k"] = {"workload": "config[3]: one %dx%d pair, %d-level pyramid, max_iter %d/level, frame 0, one step" % (w3, h3, nl3, int(blk.max_iter)),
                                    "ms_per_step": round(best * 1e3, 2), "executed_pixel_iters": round(live3),
                                    "value": round(live3 / best / 1e6, 2), "unit": "Mpixel*iters/s",
                                    "value_nominal": round(sum(prog[i].pixel_iters for i in range(nl3 - 1)) / best / 1e6, 2),
                                    "iters_executed_per_level_fine_to_coarse": [prog[i].iters_live for i in range(nl3 - 1)],
                                    "evals_per_s": round(sum(prog[i].evaluations for i in range(nl3 - 1)) / best)}
            q.clear()
            del q
        except capi.VmError as e:
            extras["config3_4k"] = {"error": str(e)[-200:]}
    return extras


def config4_plan(n_pairs, world, rank, per_batch=4, nlanes=2):
    """Who does what in config[4] (pure arithmetic: tested on CPU).  Returns (mine, chunk_of, lane_batches): the pairs of
    this rank (static block partition, SURVEY 8(e): `for config 5: 30 pairs/4 GPUs`), the solver stream (chunk) of each of
    them -- contiguous chunks, one vm_solve_batch_cons each --, and per compositor lane the batches (lists of indices into
    `mine`, <= per_batch frames = 2 per_batch systems each) it takes in turn."""
    from videomorphing_amd import dist as vdist
    mine = vdist.shard_pairs(n_pairs, world, rank)
    n = len(mine)
    nstreams = min(default_streams(n), max(1, n))
    chunk_of = [k * nstreams // max(n, 1) for k in range(n)]
    lanes = [[list(range(g0, min(g0 + per_batch, n))) for g0 in range(li * per_batch, n, per_batch * nlanes)] for li in range(nlanes)]
    return mine, chunk_of, lanes


class Config4Job(object):
    """One rank's share of BASELINE config[4]: `frame_ids` 1080p frame pairs with their point constraints and BCOND_BORDER,
    solved the way config[2] runs a rank's share -- default_streams() contexts (HIP streams, one host thread each), the
    frames in contiguous chunks, a chunk as one vm_solve_batch_cons batch (reference semantics) --, then the compositor over
    every pair: canvases uploaded from page-locked host memory (PCIe), v upscaled on the device straight from the solver
    context's pyramid (vm_frame_set_v_from_level across contexts: an event, no host sync), Poisson extension of both sides
    of `per_batch` frames per batch (2 x per_batch systems per launch) at `tol`, 9 rendered in-between frames per pair; the
    batches dealt to `nlanes` compositor lanes (contexts = streams, a host thread each: one lane's PCIe uploads and
    latency-bound coarse-grid launches hide behind the other's level-0 kernels; tools/exp/compositor_lanes.py).  The frames
    go up as RGB8 (vm_frame_upload_rgb: the extended canvases are built on the device, as Pyramid::build builds them).
    Everything it allocates is released by close() (use try / finally)."""

    def __init__(self, np, capi, morph, synth, device, blk, cons, w, h, nlev, frame_ids, imgs, rgb0, rgb1, ex, tol, per_batch=4, nlanes=2, lane0=None):
        self.np, self.capi, self.morph = np, capi, morph
        self.blk, self.cons, self.w, self.h, self.nlev, self.ex, self.tol = blk, cons, w, h, nlev, ex, tol
        self.n = len(frame_ids)
        self.per_batch, self.nlanes = per_batch, nlanes
        self.sctx, self.lane_ctx, self.own_lane_ctx, self.lane_frs, self.groups, self.pinned = [], [], [], [], [], []
        prm = morph.Parameters()
        prm.max_iter, prm.max_iter_drop_factor, prm.start_res, prm.bcond = int(blk.max_iter), blk.max_iter_drop_factor, blk.start_res, capi.BCOND_BORDER
        self.kp = morph.KernParameters(prm)
        _, self.chunk_of, self.lane_batches = config4_plan(self.n, 1, 0, per_batch, nlanes)      # (the rank's share is a job of its own)
        self.nstreams = max(self.chunk_of) + 1 if self.chunk_of else 1
        self.sctx, self.solver_streams_rejected = solver_contexts(morph, device, blk.math_mode, self.nstreams)
        for c in self.sctx:
            c.set_params(self.kp)
        self.imgs = imgs
        self.device = device
        self.lane_ctx = [lane0 if (li == 0 and lane0 is not None) else morph.Context(device, blk.math_mode) for li in range(nlanes)]
        self.own_lane_ctx = [c for c in self.lane_ctx if c is not lane0]
        self.lane_retries, self.lane_gain, self._parked = 0, None, []
        self.lane_frs = [[morph.Frame(c, w, h, ex) for _ in range(per_batch)] for c in self.lane_ctx]
        self.e0, self.e1 = morph.pin_host(rgb0), morph.pin_host(rgb1)    # the caller's RGB8 frames, page-locked (vm_host_register)
        self.pinned = [self.e0, self.e1]

    def pyramids(self):
        """a set of pyramids of the rank's frames, resident in HBM, each on its chunk's solver context"""
        group = []
        for k in range(self.n):
            q = self.morph.Pyramid(self.sctx[self.chunk_of[k]])
            q.build(self.imgs[k][0], self.imgs[k][1], self.blk.start_res, nlevels=self.nlev)
            group.append(q)
        self.groups.append(group)
        return group

    def chunks(self, group):
        return [[q for q, cix in zip(group, self.chunk_of) if cix == s] for s in range(self.nstreams)]

    def _warm_lane(self, li, group):
        for f in self.lane_frs[li]:
            f.upload_rgb(self.e0, self.e1)
            f.set_v_from_level(group[0], 1)
        self.morph.poisson_extend_frames(self.lane_frs[li], tol=1e-3)

    def _lane_probe(self, group):
        """what the second lane buys on THIS pair of streams: seconds of one batch per lane run one lane after the other / run
        side by side (the work itself is the probe)"""
        from concurrent.futures import ThreadPoolExecutor
        sub = [b[0] for b in self.lane_batches[:2]]             # the first batch of lanes 0 and 1

        def one(li):
            c, frs = self.lane_ctx[li], self.lane_frs[li]
            qs = [group[k] for k in sub[li]]
            for f, q in zip(frs, qs):
                f.upload_rgb(self.e0, self.e1)
                f.set_v_from_level(q, 1)
            self.morph.poisson_extend_frames(frs[:len(qs)], tol=self.tol)
            for f in frs[:len(qs)]:
                for k in range(1, 10):
                    f.render_halfway_dev(0.1 * k, 0.1 * k, 1)
            c.sync()
        best_seq = best_par = 1e30
        for _ in range(2):
            t0 = time.perf_counter(); one(0); one(1); best_seq = min(best_seq, time.perf_counter() - t0)
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=2) as ex_:
                list(ex_.map(one, (0, 1)))
            best_par = min(best_par, time.perf_counter() - t0)
        return best_seq / best_par

    def warm_up(self, group):
        """workspaces (schedules, graphs, the solver's hierarchy) are allocated on first use: not timed.  And the lanes are
        CHOSEN here: the runtime deals a new stream to one of its hardware queues as it likes, and on some pairs of queues two
        streams take turns instead of running side by side -- measured: the two lanes then need 3.2 instead of 2.4 ms per frame,
        in about one process out of five, whatever GPU_MAX_HW_QUEUES says; a probe with do-nothing kernels
        (vm_dbg_streams_overlap) finds the pairs that serialise outright but not all that slow the real work down.  So the
        work itself is the probe: one batch per lane, one lane after the other against side by side; a second lane that buys
        less than 15 % is replaced by a context on a fresh stream (the rejected one stays alive meanwhile, so that the next
        stream lands elsewhere), at most four times."""
        for li in range(self.nlanes):
            self._warm_lane(li, group)
        if self.nlanes == 2 and len(self.lane_batches[1]) > 0 and not os.environ.get("VM_NO_LANE_PROBE"):
            for attempt in range(5):
                self.lane_gain = self._lane_probe(group)
                if self.lane_gain >= 1.15 or attempt == 4:
                    break
                self.lane_retries += 1
                for f in self.lane_frs[1]:
                    f.close()
                self._parked.append(self.lane_ctx[1])
                c = self.morph.Context(self.device, self.blk.math_mode)
                self.lane_ctx[1] = c
                self.own_lane_ctx = [x for x in self.own_lane_ctx if x is not self._parked[-1]] + [c]
                self.lane_frs[1] = [self.morph.Frame(c, self.w, self.h, self.ex) for _ in range(self.per_batch)]
                self._warm_lane(1, group)
            for c in self._parked:
                try:
                    c.close()
                except Exception:
                    pass
            self._parked = []
        self.solve(group)

    def solve(self, group):
        """(seconds, per-pair progress lists) of the solve stage"""
        from concurrent.futures import ThreadPoolExecutor
        one = lambda ch: self.morph.solve_batch(ch, self.blk.max_iter, self.blk.max_iter_drop_factor, fixed_work=False, constraints=self.cons) if ch else []
        for c in self.sctx:
            c.sync()
        t1 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=self.nstreams) as ex_:
            res = list(ex_.map(one, self.chunks(group)))
        for c in self.sctx:
            c.sync()
        return time.perf_counter() - t1, [r for ch in res for r in ch]

    def _lane(self, grp, li, collect):
        c, frs = self.lane_ctx[li], self.lane_frs[li]
        t_up = t_po = t_re = 0.0
        its, digests = [], {}
        for batch in self.lane_batches[li]:
            g0 = batch[0]
            qs = [grp[k] for k in batch]
            t2 = time.perf_counter()
            for f, q in zip(frs, qs):
                f.upload_rgb(self.e0, self.e1)              # 12 MB over PCIe; the canvases are built on the device (pyramid.cu:186-200)
                f.set_v_from_level(q, 1)
            c.sync(); t3 = time.perf_counter()
            res, _ = self.morph.poisson_extend_frames(frs[:len(qs)], tol=self.tol)
            c.sync(); t4 = time.perf_counter()
            for j, f in enumerate(frs[:len(qs)]):
                for k in range(1, 10):
                    if collect is not None:
                        collect[(g0 + j, k)] = f.render_halfway(0.1 * k, 0.1 * k, 1)
                    else:
                        f.render_halfway_dev(0.1 * k, 0.1 * k, 1)
                if collect is not None:
                    collect[(g0 + j, "v")] = f.download_v()
            c.sync(); t5 = time.perf_counter()
            t_up += t3 - t2; t_po += t4 - t3; t_re += t5 - t4
            its += [s_[0] for r in res for s_ in r]
        return t_up, t_po, t_re, its

    def compositor(self, grp, collect=None):
        """(wall s, per-stage s on the lanes' own clocks / lanes, PCG iteration counts); collect: a dict that receives
        every rendered frame and every pair's field (tests)"""
        from concurrent.futures import ThreadPoolExecutor
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=self.nlanes) as ex_:
            parts = list(ex_.map(lambda li: self._lane(grp, li, collect), range(self.nlanes)))
        wall = time.perf_counter() - t0
        return wall, [sum(p_[k] for p_ in parts) / self.nlanes for k in range(3)], [i_ for p_ in parts for i_ in p_[3]]

    def step(self, group, collect=None):
        """the two stages in a row: {seconds, solve_s, comp_s, split, its, executed pixel*iters}"""
        t1 = time.perf_counter()
        t_solve, progs = self.solve(group)
        t_comp, split, its = self.compositor(group, collect)
        dt = time.perf_counter() - t1
        sizes = [(group[0][el].width, group[0][el].height) for el in range(1, self.nlev)]
        live = sum(float(pr[i]["iters_live"]) * sizes[i][0] * sizes[i][1] for pr in progs for i in range(self.nlev - 1))
        return {"s": dt, "solve_s": t_solve, "comp_s": t_comp, "split": split, "its": its, "pixel_iters": live}

    def overlapped(self, group, group_b):
        """a STREAM of such jobs: the compositor of job N (the lanes) runs while job N + 1 is solved on the solver streams --
        a second set of pyramids, so that the compositor reads fields nobody is writing; wall time of the overlapped pair of
        stages = the steady-state time per job"""
        from concurrent.futures import ThreadPoolExecutor
        one = lambda ch: self.morph.solve_batch(ch, self.blk.max_iter, self.blk.max_iter_drop_factor, fixed_work=False, constraints=self.cons) if ch else []
        for c in self.sctx + self.lane_ctx:
            c.sync()
        t6 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=self.nstreams + 1) as ex_:
            fs = [ex_.submit(one, ch) for ch in self.chunks(group_b)]
            fc = ex_.submit(self.compositor, group)
            for f_ in fs:
                f_.result()
            t_solve_b = time.perf_counter() - t6
            fc.result()
        for c in self.sctx + self.lane_ctx:
            c.sync()
        dt_p = time.perf_counter() - t6
        return {"ms_per_pair": round(dt_p * 1e3 / self.n, 1), "solve_ms_per_pair_while_compositing": round(t_solve_b * 1e3 / self.n, 1),
                "rendered_frames_per_s": round(self.n * 9 / dt_p, 1),
                "what": "steady state of a stream of such jobs: job N's compositor (its lanes) overlapped with job N + 1's solve (the solver streams)"}

    def close(self):
        for frs in self.lane_frs:
            for f in frs:
                try:
                    f.close()
                except Exception:
                    pass
        for group in self.groups:
            for q in group:
                try:
                    q.clear()
                except Exception:
                    pass
        for c in self.sctx + self.own_lane_ctx + self._parked:
            try:
                c.close()
            except Exception:
                pass
        for a in self.pinned:
            try:
                self.morph.unpin_host(a)
            except Exception:
                pass
        self.lane_frs, self.groups, self.sctx, self.own_lane_ctx, self.pinned = [], [], [], [], []


def config4_workload(n, nstreams, per_chunk, ex, per_batch, nlanes, tol):
    return ("config[4]: %d 1080p pairs, 8 point constraints each, BCOND_BORDER, solved on %d streams x one batch of %d (reference "
            "semantics); per frame: RGB8 frames uploaded from page-locked host memory (PCIe), canvases built and v upscaled on the device, Poisson extension (ex = %d, tol %g) of "
            "both sides, %d frames = %d systems per batch, the batches dealt to %d compositor lanes (streams); 9 rendered in-between frames per pair"
            % (n, nstreams, per_chunk, ex, tol, per_batch, 2 * per_batch, nlanes))


def pipeline30(np, capi, morph, synth, ctx, blk, w, h, nlev, rgb0, rgb1, ex, render_ms, device, frames, tol, nframes=30, per_batch=4, reps=3):
    """config[4] on one GPU (see run_extras): returns the extras entry.  The whole job `reps` times: min and median (one run
    each was what rounds 4-5 reported, and the driver's fresh box then differed from the quoted figures by 6-30 %)."""
    cons = synth.make_constraints(w, h, 8)
    ids = list(range(2000, 2000 + nframes))
    job = Config4Job(np, capi, morph, synth, device, blk, cons, w, h, nlev, ids, frames(ids), rgb0, rgb1, ex, tol, per_batch, 2, lane0=ctx)
    try:
        group = job.pyramids()
        job.warm_up(group)
        runs = [job.step(group) for _ in range(reps)]
        piped = None
        try:
            piped = job.overlapped(group, job.pyramids())
        except capi.VmError as e:
            piped = {"error": str(e)[-160:]}
        n = job.n
        best = min(runs, key=lambda r: r["s"])
        med = lambda key: statistics.median(r[key] for r in runs)
        t_up, t_po, t_re = best["split"]
        its = best["its"]
        return {"workload": config4_workload(n, job.nstreams, len(job.chunks(group)[0]), ex, per_batch, job.nlanes, tol) + "; on ONE GPU",
                "runs": reps, "what_is_quoted": "the fastest of the runs (ms_per_pair etc.); *_median beside it",
                "ms_per_pair": round(best["s"] * 1e3 / n, 1), "ms_per_pair_median": round(med("s") * 1e3 / n, 1),
                "ms_per_pair_each_run": [round(r["s"] * 1e3 / n, 1) for r in runs],
                "solve_ms_per_pair": round(best["solve_s"] * 1e3 / n, 1), "solve_ms_per_pair_median": round(med("solve_s") * 1e3 / n, 1),
                "compositor_ms_per_frame": round(best["comp_s"] * 1e3 / n, 2), "compositor_ms_per_frame_median": round(med("comp_s") * 1e3 / n, 2),
                "compositor_lanes": job.nlanes,
                # the second lane is chosen by measurement (Config4Job.warm_up): what it buys on one batch per lane, and how
                # many streams were tried and given back before that
                "second_lane_gain": job.lane_gain and round(job.lane_gain, 2), "second_lane_streams_rejected": job.lane_retries,
                # each lane's own clock per stage, summed over the lanes / lanes (the lanes run side by side)
                "compositor_split_ms_per_frame": {"upload_pcie_and_v_upscale": round(t_up / n * 1e3, 2), "poisson_both_sides": round(t_po / n * 1e3, 2),
                                                  "render_9_frames": round(t_re / n * 1e3, 2)},
                "poisson_tol": tol, "pcg_iterations_min_max": [min(its), max(its)],
                "solve_mpix_iters_per_s": round(best["pixel_iters"] / best["solve_s"] / 1e6, 1),
                # Metric 2: frames/s of render_halfway, device-resident inputs -- render only, and with the
                # Poisson extension (and the canvas upload) of the pair amortised over its 9 rendered frames
                "render_frames_per_s": {"render_only": round(1000.0 / render_ms, 1) if render_ms else None,
                                        "with_poisson_amortised": round(n * 9 / best["comp_s"], 1),
                                        "with_poisson_amortised_median": round(n * 9 / med("comp_s"), 1),
                                        "whole_pipeline_incl_solve": round(n * 9 / best["s"], 1),
                                        "whole_pipeline_incl_solve_median": round(n * 9 / med("s"), 1),
                                        "whole_pipeline_stages_overlapped": piped and piped.get("rendered_frames_per_s")},
                "stages_overlapped": piped}
    finally:
        job.close()


def sync_stage_extra(np, morph, ctx, w, h, d, blk):
    prm = morph.Parameters()
    prm.w_ui, prm.w_tps, prm.max_iter = 100.0, 0.001, int(blk.max_iter)
    rng = np.random.default_rng(23)
    for k in range(24):
        lx, ly, lz = int(rng.integers(2, w - 2)), int(rng.integers(2, h - 2)), int(rng.integers(0, d))
        prm.lp.append([morph.Conp(lx, ly, lz)])
        prm.rp.append([morph.Conp(int(np.clip(lx + rng.integers(-40, 41), 0, w - 1)), int(np.clip(ly + rng.integers(-40, 41), 0, h - 1)),
                                  int(np.clip(lz + rng.integers(-3, 4), 0, d - 1)))])
        prm.cnt.append([morph.Connect((k, 0), (k, 0))])
    levels = morph.sync_level_table(w, h, d, max(blk.start_res // 2, 1))   # UI/MdiEditor.cpp:1837
    pyr = morph.SyncPyramid(ctx)
    pyr.build_levels(levels)
    for rep in range(2):                                 # the first pass allocates the workspaces
        th = morph.SyncThread(prm, pyr)
        ctx.sync(); t1 = time.perf_counter()
        th.run()
        ctx.sync(); dt = time.perf_counter() - t1
    solve_ms = sum(pr["elapsed_ms"] for pr in th.progress.values())
    units = sum(pr["voxel_iters"] for pr in th.progress.values())
    fin = th.progress[1]
    n1 = levels[1][0] * levels[1][1] * levels[1][2]
    us = fin["elapsed_ms"] * 1e3 / max(fin["iters"], 1)
    gbs = n1 * 124.0 / (us * 1e-6) / 1e9
    out = {"levels": [list(l) for l in levels[1:]], "cg_iterations": [th.progress[el]["iters"] for el in sorted(th.progress)],
           "solve_ms": round(solve_ms, 1), "wall_ms_with_result_delivery": round(dt * 1e3, 1),
           "mvoxel_iters_per_s": round(units / solve_ms / 1e3, 1),
           "finest_level": {"voxels": n1, "us_per_iteration": round(us, 1), "algorithmic_bytes_per_voxel_iter": 124,
                            "achieved_GBps": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3)}}
    # stage-1 renderer on 8 of the frames (render_resample_image): both videos re-timed
    frame = np.zeros((h, w, 4), np.uint8)
    frame[..., 0] = (np.arange(w) % 256)[None, :]
    frame[..., 1] = (np.arange(h) % 256)[:, None]
    flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0] = 1.5
    for side in range(2):
        for t in range(d):
            pyr.upload_frame(side, t, frame)
            pyr.upload_flow(side, t, flow)
    ms = []
    for f in range(8):
        ms.append(pyr.render_resample_dev(0.0, f) + pyr.render_resample_dev(1.0, f))   # MdiEditor::NextStage: both sides per frame
    out["resample_ms_per_frame_both_videos"] = round(float(np.median(ms[1:])), 3)
    pyr.clear()
    return out


DUMP_MAX_BYTES = 64 << 20
DUMP_SEED = 20240601


def dump_plan(arrays, max_bytes=DUMP_MAX_BYTES):
    """`--dump-outputs`: name -> array as written.  Floating arrays stay float32 / go to float64, anything else becomes
    float64.  If everything together exceeds max_bytes, every array of more than 2^20 elements is replaced by
    `<name>_sample`, a fixed, seeded sample of its flattened elements (the same positions for the same shape in every run),
    with `<name>_sample_index` (float64 flat indices) beside it; the sample sizes are chosen so that the total fits."""
    import numpy as np
    conv = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        conv[name] = a.astype(np.float32 if a.dtype == np.float32 else np.float64, copy=False)
    if sum(a.nbytes for a in conv.values()) <= max_bytes:
        return conv
    big = [n for n, a in conv.items() if a.size > (1 << 20)]
    rest = sum(a.nbytes for n, a in conv.items() if n not in big)
    frac = max(max_bytes - rest, 0) / float(sum(conv[n].size * (conv[n].itemsize + 8) for n in big))
    out = {n: a for n, a in conv.items() if n not in big}
    for n in big:
        a = conv[n].ravel()
        k = int(a.size * frac)
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, size=k, replace=False))
        out[n + "_sample"] = a[idx]
        out[n + "_sample_index"] = idx.astype(np.float64)
    return out


def dump_outputs(path, arrays, rank=None):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in dump_plan(arrays).items():
        np.save(os.path.join(path, name + ("_rank%d" % rank if rank else "") + ".npy"), a)


def effective_cpus():
    """CPUs this process may actually use: affinity mask capped by the cgroup quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except Exception:
            pass
    return n


def cpu_baseline(np, capi, L, blk, gps, nlev, ctx):
    """The CPU restatement (oracle, OpenMP over tiles) timed on this host on a bounded sample
    of the same workload, and the GPU timed on the IDENTICAL sample beside it: every level of
    a solve (coarsest first, incl. the 120x68 one), each started -- like the solver does -- from
    the upsampled solution of the next coarser level and swept with reference semantics (stop
    when no pixel improved) for at most max_iter iterations or 8 s of CPU time; pair after pair
    of the run's first three until 10 s of CPU work are in (bounded at ~25 s); the GPU then runs
    exactly the iterations the CPU ran, from the same start -- once in the quoted arithmetic
    (timed: gpu_same_sample) and once in EXACT arithmetic, whose halfway field is compared with
    the oracle's bit for bit (parity_same_sample)."""
    import oracle as O
    threads = effective_cpus()
    O.lib().vmo_set_threads(threads)
    P = O.default_params()
    for f, _ in P._fields_:
        if hasattr(blk.kp, f):
            setattr(P, f, getattr(blk.kp, f))
    stats = np.zeros(4)
    units, spent, gpu_ms, exact_ms, parts = 0.0, 0.0, 0.0, 0.0, []
    identical, max_dv, words_diff = True, 0.0, 0
    mode0 = blk.math_mode
    npairs = 0
    for gp, el in [(g, e) for g in gps for e in range(nlev - 1, 0, -1)]:   # el = python-side level index, nlev = coarsest (host-solved)
        if spent > 25.0 or (el == nlev - 1 and spent > 10.0):
            break
        npairs += el == nlev - 1
        w, h = gp[el].width, gp[el].height
        coarse = O.Level(gp[el + 1].width, gp[el + 1].height)
        coarse.field("v")[...] = gp[el + 1].v
        tgt = O.Level(w, h)
        tgt.set_images(gp[el].field("img0"), gp[el].field("img1"))
        tgt.upsample_from(coarse)
        tgt.init(P.ssim_clamp)
        t0 = time.perf_counter()
        iters = 0
        while time.perf_counter() - t0 < 8.0 and iters < int(blk.max_iter):
            imp = tgt.optimize_iter(P, stats)
            iters += 1
            if not imp:
                break
        spent += time.perf_counter() - t0
        units += float(w) * h * iters
        parts.append(("| " if el == nlev - 1 and parts else "") + "%dx%d:%d" % (w, h, iters))
        # the GPU on the same sample: same start, reference semantics, the CPU's iteration count
        for mode in (mode0, capi.MATH_EXACT):      # EXACT last: the next finer level starts from the oracle's own field
            ctx.set_math_mode(mode)
            capi.check(L.vm_upsample_v(gp._h, el - 1, el))
            capi.check(L.vm_init_level(gp._h, el - 1, gp[1].width, gp[1].height, None, 0))
            pr = capi.Progress()
            t1 = time.perf_counter()
            capi.check(L.vm_optimize_level(gp._h, el - 1, float(iters), None, 0, C.byref(pr)))
            dt = (time.perf_counter() - t1) * 1e3
            if mode == mode0:
                gpu_ms += dt
            if mode == capi.MATH_EXACT:
                exact_ms += dt
                a, b = tgt.field("v"), gp[el].v
                nd = int((a.view(np.uint32) != b.view(np.uint32)).sum())
                words_diff += nd
                identical = identical and nd == 0 and pr.iters == iters
                max_dv = max(max_dv, float(np.abs(a - b).max()))
    ctx.set_math_mode(mode0)
    cpu_rate = units / spent / 1e6
    gpu_rate = units / (gpu_ms * 1e-3) / 1e6
    return {"value": round(cpu_rate, 3), "unit": "Mpixel*iters/s",
            "cores": threads, "kind": "port",
            "sample": "reference-semantics sweeps of levels [%s] (coarse to fine, each from the upsampled coarser solution) of the "
                      "first %d pair(s) of the run (oracle, OpenMP over tiles, %d threads), %.1f s; %.0f energy evaluations" % (
                          ", ".join(parts).replace(", |", " |"), npairs, threads, spent, stats[3]),
            "note": "compare with gpu_same_sample (the identical sample: same levels, starts and iteration counts), not with `value` "
                    "(other frames, the solver's own schedule of levels)",
            "gpu_same_sample": {"value": round(gpu_rate, 2), "unit": "Mpixel*iters/s", "ms": round(gpu_ms, 2),
                                "ratio_to_cpu": round(gpu_rate / max(cpu_rate, 1e-9), 1),
                                "note": "the HIP path on the identical sample: same levels, same starts, same iteration counts "
                                        "(wall time incl. launches and flag read-backs)"},
            "parity_same_sample": {"bit_identical": bool(identical), "max_abs_dv": max_dv, "words_differing": words_diff,
                                   "exact_ms": round(exact_ms, 2),
                                   "note": "EXACT arithmetic on the identical sample vs the oracle: halfway field of every level, "
                                           "bit for bit, and the iteration counts"}}


if __name__ == "__main__":
    main()
