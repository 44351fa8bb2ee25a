/*
 * vmorph.h -- C-ABI of the MI355X-native halfway-domain morph solver.
 *
 * This is the drop-in boundary for the hot path of liaojing/videomorphing:
 * the entry points below are what a binding of the reference's L3 solver API
 * (Algorithm/morph.h, Pyramid.h, parameters.h; UI/RenderWidget.h:52-57;
 * Algorithm/PoissonExt.h) would call.  Each declaration cites the reference
 * interface it replaces (paths relative to the reference repository).
 * INTEGRATION.md shows the reference-side stubs.
 *
 * Conventions
 *  - extern "C", opaque handles, plain pointers and sizes; no exceptions
 *    cross the ABI.  Every function returns VM_OK (0) or a negative VM_E_*
 *    code; vm_last_error() returns a thread-local message for the last error.
 *    (The reference throws std::runtime_error from rod::check_cuda_error,
 *    include/util/error.cpp:9-23; the C++ facade re-raises from these codes.)
 *  - One vm_ctx per device and host thread; all work of a context is
 *    stream-ordered on the context's HIP stream.  The caller owns host memory,
 *    the context owns device memory.
 *  - One vm_pyr holds ONE frame pair (a depth-1 pyramid: the independent-pair
 *    formulation of BASELINE.json; the reference's temporal coupling,
 *    morph.cu:1394-1439, is out of scope).  Level 0 is the finest level, level
 *    nlevels-1 the coarsest one, which only ever holds `v` (it is solved
 *    densely on the host, morph.cu:152).
 *  - Images and fields cross the boundary as tight or pitched row-major host
 *    arrays; `pitch` counts ELEMENTS of the array's scalar type per row
 *    (floats), 0 meaning tight.  float2 fields are interleaved (x,y).
 *  - There is no CPU fallback: if the HIP device or the code object is
 *    missing, vm_ctx_create fails with VM_E_DEVICE.
 */
#ifndef VMORPH_H
#define VMORPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VM_OK            0
#define VM_E_INVALID    -1   /* bad argument */
#define VM_E_DEVICE     -2   /* HIP error (message in vm_last_error) */
#define VM_E_STATE      -3   /* call out of order (e.g. optimize before init) */
#define VM_E_NUMERIC    -4   /* coarse solve / Poisson solve failed */
#define VM_E_CANCELLED  -5   /* run_flag went to 0 */

typedef struct vm_ctx vm_ctx;
typedef struct vm_pyr vm_pyr;

/* enum BoundaryCondition, Algorithm/parameters.h:9-14 */
enum { VM_BCOND_NONE = 0, VM_BCOND_CORNER = 1, VM_BCOND_BORDER = 2 };

/* struct KernParameters, Algorithm/parameters.h:54-72 (same fields, same order) */
typedef struct {
    float w_temp, w_ui, w_tps, w_ssim;
    float ssim_clamp;
    float eps;
    int   bcond;
} vm_kern_params;

/* One connected point pair (Parameters::lp/rp/cnt, parameters.h:16-27, 45-47)
 * resolved by the caller to full-resolution pixel indices, as consumed at
 * Algorithm/morph.cu:357-366: weight = MIN(weight_l, weight_r). */
typedef struct {
    float lx, ly, rx, ry;
    float weight;
} vm_constraint;

/* arithmetic mode of the optimizer kernels */
enum {
    VM_MATH_EXACT = 0,  /* IEEE +,-,*,/,sqrt, no contraction: bit-identical to the CPU oracle */
    VM_MATH_FAST  = 1,  /* fused multiply-add, v_rcp/v_sqrt approximations: the
                           analogue of the reference's --use_fast_math build
                           (MdiEditor.vcxproj:208-213) */
    VM_MATH_EXACT_FMA = 2, /* diagnostic: the EXACT source compiled with -ffp-contract=fast --
                           fused multiply-adds wherever the compiler contracts, IEEE division
                           and square root -- i.e. what nvcc's default --fmad=true makes of the
                           reference source WITHOUT --use_fast_math: one more legal rounding of
                           the same algorithm (sweep kernels only; not bit-comparable to the
                           oracle), used to measure the reproducibility floor FAST is judged
                           against (tests/test_gpu_fullsize.py) */
    VM_MATH_REF_FASTMATH = 3, /* diagnostic: the EXACT source as the reference's project file compiles
                           it -- --use_fast_math (MdiEditor.vcxproj:208-213): contraction plus
                           approximate division (x * rcp(y), CUDA's __fdividef) and square root.  The
                           reference's own expressions in the reference's own arithmetic: the third
                           member of the family of legal builds */
    VM_MATH_REF_TEX8 = 4,  /* diagnostic: the EXACT source (IEEE, no contraction) with every texture
                           fetch -- both images, Algorithm/morph.cu:29-30, 316-322 (taps at :212-213,
                           680-681, 960-961), and the inter-level upsample, include/util/
                           imgop_upsample.cu:17-31 -- filtered with CUDA's 9-bit fixed-point bilinear
                           weights (8 fractional bits, rounded to nearest): the one piece of the
                           reference BINARY's arithmetic no other mode has; the finite-difference
                           step eps = 0.01 px is 2.56 weight quanta.  The CPU checker under tests/ has
                           the same switch; the two agree bit for bit */
    VM_MATH_REF_TEX8_TRUNC = 5 /* the same with truncated weights (the CUDA guide does not state the
                           rounding rule): sensitivity check */
};

/* progress of one optimize_level call; mirrors the public progress members of
 * class Morph (Algorithm/morph.h:19-20) */
typedef struct {
    int    iters;          /* iterations executed (4 tile-offset sweeps each)  */
    int    improving;      /* 1 if the last executed iteration still improved  */
    double pixel_iters;    /* iters * W * H  (morph.cu:1389)                    */
    float  elapsed_ms;     /* HIP-event time of the sweep kernels on the stream */
    int    launches;       /* sweep kernel launches enqueued                    */
    double active_tiles;   /* tile visits that were not skipped by the mask     */
    double candidates;     /* pixel visits that ran the line search             */
    double commits;        /* accepted moves                                    */
    double evaluations;    /* energy evaluations executed (each: 2 bilinear taps
                              + 25 SSIM terms, morph.cu:671-761)                 */
    /* HIP-event time and launch count of the sweep kernels per schedule:
     * [0] TILE, dense kernel; [1] TILE, lean kernel (pruned sweeps); [2] STEP / SPLIT;
     * [3] SPARSE; [4] PASS */
    float  sched_ms[5];
    int    sched_launches[5];
    /* iterations up to and including the first that accepted no move: what the reference's
     * stopping rule (morph.cu:1390) executes.  A fixed-work run reports iters = max_iter; the
     * iters - iters_live sweeps past convergence are provable no-ops (every mask bit is clear)
     * and are skipped on the device. */
    int    iters_live;
    /* in-kernel clock probe: the first workgroup of every launch of the dense TILE kernel ([0]) and of the PASS
     * kernel ([1]) brackets its sweep with s_memtime (shader cycles) and s_memrealtime (constant 100 MHz); the
     * sums over the call's launches.  clk_shader_ticks / clk_wall_ticks x 100 MHz = the shader clock the chip
     * actually held inside that kernel (0 / 0: the schedule did not run). */
    double clk_shader_ticks[2];
    double clk_wall_ticks[2];
} vm_progress;

/* device-state arrays a test or a UI may read back (vm_level_get_field) */
enum {
    VM_F_IMG0 = 0, VM_F_IMG1, VM_F_V, VM_F_LUMA, VM_F_MEAN, VM_F_VAR, VM_F_CROSS,
    VM_F_VALUE, VM_F_COUNTER, VM_F_TPS_AXY, VM_F_TPS_B, VM_F_UI_AXY, VM_F_UI_B,
    VM_F_IMPMASK,
    /* pages of a video (vm_video_get_field): lvl.temp.ref (float2), lvl.temp.mask, the four
     * flow fields of the page (float2) */
    VM_F_TEMP_REF, VM_F_TEMP_MASK, VM_F_FLOW_F0, VM_F_FLOW_F1, VM_F_FLOW_B0, VM_F_FLOW_B1
};

const char *vm_last_error(void);
const char *vm_version(void);

/* ---- context ------------------------------------------------------------- */
/* replaces MdiEditor::CudaInit device selection, UI/MdiEditor.cpp:54-75 */
int  vm_ctx_create(int device, vm_ctx **out);
void vm_ctx_destroy(vm_ctx *ctx);
int  vm_ctx_sync(vm_ctx *ctx);
/* copy_to_symbol(c_params, KernParameters), Algorithm/morph.cu:1355-1358 */
int  vm_set_params(vm_ctx *ctx, const vm_kern_params *p);
int  vm_get_params(vm_ctx *ctx, vm_kern_params *p);
int  vm_set_math_mode(vm_ctx *ctx, int mode);
/* scheduling of the sweep (results do not depend on it): VM_SWEEP_TILE = one launch
 * per tile-offset pass, one workgroup per tile; VM_SWEEP_SPLIT = two launches per
 * phase (line searches, then the commit), a tile's candidates spread over `parts`
 * workgroups (small levels); VM_SWEEP_STEP = one launch per phase, the commit of a
 * phase folded into the next phase's launch; VM_SWEEP_SPARSE = TILE, but every batch of
 * iterations of a pruned level (fewer than a tenth of the pixels searched) runs as ONE launch
 * in which one workgroup per pair walks the active tiles; VM_SWEEP_PASS = one launch per
 * pass for small levels: a tile's four phases stay inside the launch, its 32 workgroups (one
 * wave per phase pixel) meet at a tile-local barrier between phases; VM_SWEEP_AUTO picks per
 * batch of iterations.
 * threads/parts: 0 = automatic.  `parts` of a FORCED schedule (tests): SPLIT / STEP = workgroups per tile; SPARSE = the
 * LDS capacity of the kernel's word list; PASS = 1: write-through stores from the start, 2: tile groups spread over
 * the XCDs; TILE (FAST) = from how many workgroups per pass (tiles x pairs) a pruned pass takes its listed form -- a
 * scan of the mask lists the tiles a set bit reaches, a fixed grid of workgroups walks the list; 0 = 4096. */
enum { VM_SWEEP_AUTO = 0, VM_SWEEP_TILE = 1, VM_SWEEP_SPLIT = 2, VM_SWEEP_STEP = 3, VM_SWEEP_SPARSE = 4, VM_SWEEP_PASS = 5 };
int  vm_set_tuning(vm_ctx *ctx, int sweep_mode, int threads, int parts);
/* Diagnostic, EXACT arithmetic only: the order in which the commits of one Jacobi phase are
 * folded into the shared window sums.  The reference leaves it to float atomics
 * (morph.cu:951-1015); the oracle and this library fix it as row-major over the committing
 * pixels (order 0).  order 1 applies that sequence reversed, 2 column-major, 3 column-major
 * reversed -- equally legal trajectories, used to measure how far legal runs drift apart
 * (the per-frame chaos floor FAST is judged against, tests/test_gpu_fullsize.py).  Other
 * values: VM_E_INVALID. */
int  vm_set_commit_order(vm_ctx *ctx, int order);
/* How the compositor's linear solver -- the batched multigrid PCG behind vm_poisson_extend, vm_poisson_extend_frames and
 * vm_frame_quadratic_path -- and the quadratic path's mean shift add up their dot products.  The reference extends by a
 * direct sparse solve (MKL DSS, PoissonExt.cpp:321-329): one answer per input.
 *   VM_REDUCE_ATOMIC  (default) one double atomic per workgroup and channel: the sum order is arrival order, so two
 *                     runs -- or one frame alone and in a batch -- may stop an iteration apart and differ by a level
 *                     on some bytes;
 *   VM_REDUCE_ORDERED every sum is a fold in ONE fixed order that depends on the system alone (its own block and tile
 *                     lists): the same bytes, iteration counts and residual bits from run to run, process to
 *                     process, alone or in any batch, on any context.  (The development switch VM_MGB_FUSE_MIN_SYS
 *                     moves the PCG update between two kernels that partition level 0 differently -- by tiles, by
 *                     blocks: the ordered bits of the two settings may differ.)
 * Contexts the library creates on behalf of this one (the lanes of vm_video_solve) inherit the mode.  The environment
 * variable VM_REDUCTION=ordered|atomic sets the mode a context starts with (any other value: vm_ctx_create fails
 * with VM_E_INVALID).  A NULL context or another mode: VM_E_INVALID. */
#define VM_REDUCE_ATOMIC 0
#define VM_REDUCE_ORDERED 1
int  vm_set_reduction(vm_ctx *ctx, int mode);
/* Test hooks of the PASS schedule's safety net.  k_pass spins at tile-local barriers with a bounded
 * wait; under VM_SWEEP_AUTO a timeout (compute units masked away or held by someone else) restores the
 * level to where the batch of iterations started, reruns the batch with the STEP schedule and keeps the
 * context off PASS from then on; a forced VM_SWEEP_PASS reports VM_E_DEVICE.  force_timeout(on != 0)
 * makes one workgroup of every following PASS launch walk away from its tile group, so that the rest
 * times out for real (2 s); on == 0 ends that and re-admits PASS.  fallbacks = how many batches this
 * context has rerun with STEP. */
int  vm_dbg_pass_force_timeout(vm_ctx *ctx, int on);
int  vm_dbg_pass_fallbacks(vm_ctx *ctx);
/* Test hook of the SPARSE schedule's resident visits (FAST arithmetic): while the set bits
 * of a pruned level's improving mask fit one tile, k_sparse keeps the window sums around them in LDS across passes
 * and iterations instead of staging and writing back a tile per pass (kernel_optimize_level's LoadSSIM / SaveSSIM,
 * morph.cu:1214-1256, once per residency instead of once per visit) -- the same bits as list-driven visits.
 * mode 0 = automatic (default), 1 = never, 2 = the LDS copy is re-centred after every commit, 3 = residency is given
 * up at the first commit (the two exits a growing active region takes, forced).  Other values: VM_E_INVALID. */
int  vm_dbg_sparse_resident(vm_ctx *ctx, int mode);
/* ... and how many tile visits of this context's solves were served from that LDS copy so far (saturating). */
int  vm_dbg_sparse_resident_visits(vm_ctx *ctx);
/* Test hook of the sweep variants (FAST arithmetic): every FAST sweep kernel exists twice, the
 * general one, which reads from the level whether its pages carry the temporal term, and one compiled without the
 * term, which the solver launches for levels that carry none -- the same bits.  mode 0 = by the level (default),
 * 1 = always the general kernels (tests, and timing one against the other inside one library).  Per context; the other
 * arithmetics have the general kernels only.  Other values: VM_E_INVALID. */
int  vm_dbg_sweep_variant(vm_ctx *ctx, int mode);
/* Diagnostic of the PASS schedule: on which XCD (0..7) each of the first `n` (<= 2048)
 * workgroups of the most recent PASS launch ran (workgroup b belongs to tile group
 * (b / 256) * 8 + b % 8; a group whose 32 workgroups report one XCD keeps its tile in one
 * L2).  The first call only arms the recording (xcc_of_block is filled with 0xFF); placement
 * is a matter of speed, never of correctness. */
int  vm_dbg_pass_placement(vm_ctx *ctx, uint8_t *xcc_of_block, int n);
/* Test hook of the wave-wide line search of the FAST sweeps (decide64): the control flow of its golden-section
 * search alone -- initial pair, regime loop, generic loop, final choice, the same text the sweep kernels expand --
 * with the energy f(t) = (A (t - t0)) (t - t0) + B in place of the taps and the SSIM change.  n cases (1 to 65536)
 * in one launch, a wave each; params: cc, A, t0, B per case (4 n floats, host; cc in [0, 16]), eps in [2^-10, 1]
 * (the bounds keep the search finite).  out, per case 20 words (host): the bits of tmin and of fmin, the count of
 * used evaluations, then the bits of the used evaluation points in order (at most 17, the rest 0).  It moves no
 * texture and touches no level state.  Bad arguments: VM_E_INVALID. */
int  vm_dbg_golden(vm_ctx *ctx, int n, const float *params, float eps, uint32_t *out);
/* Test hook of the same search's sampling: along a search line the points of the regime are known before any energy
 * is, and the four octets of each half of the wave sample four of them in one pass (the ladder); a round takes its
 * lumas from the octet that holds them.  This runs that search text on the energy f(t) = t, under which it walks the
 * whole ladder from cc down to eps, on two small images (w x h floats each, host; 2 to 64 a side), and returns what
 * the ladder delivered beside what the one-point taps of the generic loop sample at the same point.  n cases (1 to
 * 65536) in one launch, a wave each; params per case (8 n floats, host): the pixel (px, py; whole numbers inside the
 * image), the field value (vx, vy; any float), a direction (gx, gy), cc in [0, 16], one unused; eps in [2^-10, 1].
 * out, per case 201 words (host): the count of points, then per point in search order (at most 40, the rest 0) the
 * bits of t, of the ladder's (lx, ly) and of the one-point taps' (lx, ly).  Bad arguments: VM_E_INVALID. */
int  vm_dbg_ladder(vm_ctx *ctx, int w, int h, const float *img0, const float *img1, int n, const float *params,
                   float eps, uint32_t *out);
/* Do the streams of two contexts of one device run side by side?  (The reference has one device context and one stream,
 * UI/MdiEditor.cpp:54-75; a host of this library keeps several: solver streams, compositor lanes.)  The HIP runtime
 * multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues, and two streams on one queue run their kernels
 * one after the other; which queue a new stream gets is not the caller's to choose.  *overlap = 1 if a 100 us do-nothing
 * kernel on each stream overlaps the other's, 0 if they serialise.  A host that needs the overlap creates another context
 * when the answer is 0 (keeping the rejected one alive meanwhile, so that the next stream gets another queue). */
int  vm_dbg_streams_overlap(vm_ctx *a, vm_ctx *b, int *overlap);
/* Diagnostic of the device pyramid builder: scale() of include/resample as vm_pyramid_build_rgb and the flow pyramid
 * drive it (scale.cpp:225-272), on its own.  planes: 3 tight planar float planes of w x h (host), out: 3 planes of
 * wout x hout (host); any side from 1 to 16384.  The public entries reach scale() only between load and store. */
int  vm_dbg_pyramid_scale(vm_ctx *ctx, const float *planes, int w, int h, int wout, int hout, float *out);
/* device facts for reports: name (<=255 chars), CU count, HBM bytes */
int  vm_device_info(vm_ctx *ctx, char *name256, int *cus, uint64_t *hbm_bytes);

/* ---- pyramid / levels ---------------------------------------------------- */
/* Pyramid::append_new + PyramidLevel ctor, Algorithm/pyramid.cu:525-543 */
int  vm_pyramid_create(vm_ctx *ctx, int nlevels, const int *w, const int *h, vm_pyr **out);
/* Pyramid::clear, Algorithm/pyramid.cu:19-49 */
void vm_pyramid_destroy(vm_pyr *pyr);
int  vm_pyramid_levels(vm_pyr *pyr);
int  vm_level_dims(vm_pyr *pyr, int lvl, int *w, int *h, int *rowstride);
/* the cudaMemcpy2DToArray uploads of luma in Pyramid::build, pyramid.cu:275-280 */
int  vm_level_upload_luma(vm_pyr *pyr, int lvl, const float *img0, const float *img1, int pitch);
/* the image half of Pyramid::build(video0, video1, ..., start_res),
 * Algorithm/pyramid.cu:166-485, for one pair of RGB8 frames of the level-0 size:
 * load -> per level scale() (include/resample: cubic B-spline generalized sampling)
 * -> store_gray, all on the device; fills img0/img1 of every level that holds images */
int  vm_pyramid_build_rgb(vm_pyr *pyr, const uint8_t *rgb0, const uint8_t *rgb1, int pitch_bytes);
/* lvl.v.copy_from_host, Algorithm/morph.cu:588 */
int  vm_level_set_v(vm_pyr *pyr, int lvl, const float *v_xy, int pitch);
/* the cudaMemcpy2D of CMatchingThread::update_result, MatchingThread.cpp:38-40 */
int  vm_level_get_v(vm_pyr *pyr, int lvl, float *v_xy, int pitch);
/* read back any state array, tight rows: float (h*w), float2 (h*w*2) or, for
 * VM_F_IMPMASK, uint32 ((h+4)/5+2) x ((w+4)/5+2) */
int  vm_level_get_field(vm_pyr *pyr, int lvl, int field, void *host);
/* Morph::clear_level, Algorithm/morph.cu:392-414 */
int  vm_level_clear(vm_pyr *pyr, int lvl);
/* Test hook: overwrite the improving mask of an initialised level (init_improving_mask's array, morph.cu:203-260; the
 * layout vm_level_get_field(VM_F_IMPMASK) returns: ((h + 4) / 5 + 2) rows of (w + 4) / 5 + 2 words, bit x % 5 + 5 (y % 5) of
 * word (y / 5 + 1, x / 5 + 1)).  Any mask is a legal state -- it only says which pixels the next sweep searches -- so tests
 * plant small clusters of set bits to drive the schedules through their pruned regimes. */
int  vm_dbg_level_set_mask(vm_pyr *pyr, int lvl, const uint32_t *words);

/* ---- solver -------------------------------------------------------------- */
/* Morph::cpu_optimize_level, Algorithm/morph.cu:419-590 (host banded solve of
 * the coarsest level, result uploaded to the level's v) */
int  vm_coarse_solve(vm_pyr *pyr, int lvl, int w0, int h0, const vm_constraint *c, int n);
/* upsample(PyramidLevel&dest, PyramidLevel&orig), Algorithm/upsample.cu:260-286 */
int  vm_upsample_v(vm_pyr *pyr, int dst_lvl, int src_lvl);
/* Morph::initialize_level, Algorithm/morph.cu:264-390: window sums, SSIM value,
 * TPS linearisation, improving mask, and the UI-constraint splat (done on the
 * device; w0,h0 = full-resolution size the constraint coordinates refer to) */
int  vm_init_level(vm_pyr *pyr, int lvl, int w0, int h0, const vm_constraint *c, int n);
/* Morph::optimize_level, Algorithm/morph.cu:1353-1391.  Runs until no pixel
 * improves, iter >= max_iter, or *run_flag == 0 (may be NULL).  fixed_work != 0
 * ignores the convergence exit (always max_iter iterations). */
int  vm_optimize_level(vm_pyr *pyr, int lvl, float max_iter, volatile const int *run_flag,
                       int fixed_work, vm_progress *out);
/* Morph::calculate_halfway_parametrization, Algorithm/morph.cu:150-168: the
 * whole coarse-to-fine solve.  per_level (may be NULL) receives nlevels-1
 * entries, index = level. */
int  vm_solve(vm_pyr *pyr, float max_iter, float max_iter_drop_factor,
              const vm_constraint *c, int n, volatile const int *run_flag,
              int fixed_work, vm_progress *per_level);
/* The same two calls for a BATCH of frame pairs that share one context and one geometry
 * (no constraints): every sweep launch covers all pairs, which is how levels too small to
 * occupy the GPU are filled -- the natural parallelism of the path is across pairs.
 * out / per_level: n entries resp. n*(nlevels-1) entries, pair-major; elapsed_ms and
 * launches are those of the batch.  Each pair converges on its own flags. */
int  vm_optimize_level_batch(vm_pyr **pyrs, int n, int lvl, float max_iter,
                             volatile const int *run_flag, int fixed_work, vm_progress *out);
int  vm_solve_batch(vm_pyr **pyrs, int n, float max_iter, float max_iter_drop_factor,
                    volatile const int *run_flag, int fixed_work, vm_progress *per_level);
/* the same with every pair's own user constraints (Parameters::lp/rp/cnt of its frame, resolved as for
 * vm_solve: Algorithm/morph.cu:345-388, 471-505): cons[i] / ncons[i], cons == NULL = none anywhere */
int  vm_solve_batch_cons(vm_pyr **pyrs, int n, float max_iter, float max_iter_drop_factor,
                         const vm_constraint *const *cons, const int *ncons,
                         volatile const int *run_flag, int fixed_work, vm_progress *per_level);
/* CMatchingThread::update_result + Resize, Algorithm/MatchingThread.cpp:22-100:
 * v of level `lvl` scaled by (W0/W, H0/H) and bilinearly resized to w0 x h0 */
int  vm_upscale_result(vm_pyr *pyr, int lvl, int w0, int h0, float *v_xy_out, int pitch);

/* ---- video pairs: the temporal coherence path ------------------------------ */
/* The reference couples the frames of a video: class Pyramid with
 * depth > 1 -- per level `depth` pages (Algorithm/Pyramid.h:52-98) and four optical-flow
 * fields per page (f0/f1: forward flow of video 0/1 from frame t to t+1, b0/b1: backward,
 * Pyramid.h:85-90) -- and Morph::optimize_level solves the middle page first, then two
 * chains outward, each page tied to its solved neighbour by w_temp |v - ref|_1
 * (Algorithm/morph.cu:752-759, 1394-1439), ref being the neighbour's field advected along
 * the flows (initialize_temp, Algorithm/upsample.cu:214-258).  vm_video is that object; a
 * page is the same device state as a frame pair and is swept by the same kernels. */
typedef struct vm_video vm_video;
/* a connected point pair with the frame it belongs to (Conp::p.z, parameters.h:22-26) */
typedef struct {
    float lx, ly, rx, ry;
    float weight;
    int   frame;
} vm_video_constraint;
/* Pyramid::append_new per level with its depth (pyramid.cu:220-240, 462-477).  Level 0 is
 * the finest; the last level holds only v.  d[l] = pages of level l (not growing with l);
 * factor_t[l] (may be NULL: 2 where the depth shrank) = temporal stride level l was built
 * with (pyramid.cu:468); depth0 = frames of the video (the placeholder level's depth). */
int  vm_video_create(vm_ctx *ctx, int nlevels, const int *w, const int *h, const int *d,
                     const int *factor_t, int depth0, vm_video **out);
void vm_video_destroy(vm_video *v);
int  vm_video_levels(vm_video *v);
int  vm_video_level_dims(vm_video *v, int lvl, int *w, int *h, int *depth, float *factor_d);
/* the uploads of Pyramid::build for one page: lumas (pyramid.cu:275-280) and the four flow
 * fields, tight or pitched (h, w, 2) floats (pyramid.cu:323-326, 452-455); NULL = keep */
int  vm_video_upload_luma(vm_video *v, int lvl, int page, const float *img0, const float *img1, int pitch);
int  vm_video_upload_flows(vm_video *v, int lvl, int page, const float *f0, const float *f1,
                           const float *b0, const float *b1, int pitch);
/* Pyramid::build(video0, video1, f0, f1, b0, b1, start_res), pyramid.cu:166-485, on the
 * device: the image half for one frame (its luma pyramid goes to every page that shows it),
 * and the flow half for the whole video (scale, x size ratio, temporal concatenation where
 * the depth halves): f0[t].. = tight (h0, w0, 2) float arrays of the depth0 frames */
int  vm_video_build_rgb(vm_video *v, int frame, const uint8_t *rgb0, const uint8_t *rgb1, int pitch_bytes);
int  vm_video_build_flows(vm_video *v, const float *const *f0, const float *const *f1,
                          const float *const *b0, const float *const *b1);
int  vm_video_set_v(vm_video *v, int lvl, int page, const float *v_xy, int pitch);
int  vm_video_get_v(vm_video *v, int lvl, int page, float *v_xy, int pitch);
int  vm_video_get_field(vm_video *v, int lvl, int page, int field, void *host);
/* CMatchingThread::update_result for depth > 1, MatchingThread.cpp:22-84: every page of level
 * `lvl` scaled by (w0 / w, h0 / h) and resized to w0 x h0 into frame min(page * factor,
 * depth0 - 1), factor = factor_d[placeholder] / factor_d[lvl]; the frames the temporal
 * pyramid skipped are blended linearly from the two frames around them.  vm_video_result
 * delivers all depth0 frames (tight (depth0, h0, w0, 2) floats).  A level whose last page
 * stops short of the last frame ((depth - 1) * factor < depth0 - 1: never with the reference's
 * own depth tables) is refused with VM_E_STATE -- the reference would leave those frames as an
 * earlier delivery wrote them; vm_frame_set_v_from_video leaves ONE of them in a compositor frame's v, on the
 * device (w0 x h0 = the frame's size, depth0 = the depth the video was created with). */
int  vm_video_result(vm_video *v, int lvl, int w0, int h0, float *v_xy_frames);
/* Morph::cpu_optimize_level for every page of the coarsest level, morph.cu:419-590 */
int  vm_video_coarse_solve(vm_video *v, const vm_video_constraint *c, int n);
/* upsample(pyr[dst], pyr[dst+1]), upsample.cu:260-340: the spatial upsample of every coarse
 * page and, where the depth doubles, the in-between pages splatted from their two
 * neighbours along the flows, smoothed and hole-filled (temp_ref, interpolate_temp_ref,
 * smooth, fill_zeros_x; fill_zeros_y has no effect on the result) */
int  vm_video_upsample(vm_video *v, int dst_lvl);
/* Morph::initialize_level for every page, morph.cu:264-390 */
int  vm_video_init_level(vm_video *v, int lvl, const vm_video_constraint *c, int n);
/* initialize_temp(lvl, page, dir), upsample.cu:214-258: temp.ref / temp.mask of `page` from
 * page + dir (dir = -1: along its forward flows, +1: backward); the page is then swept
 * with flag == true */
int  vm_video_initialize_temp(vm_video *v, int lvl, int page, int dir);
/* Morph::optimize_level, morph.cu:1353-1441: middle page, then both chains (step k of the two
 * chains shares its launches).  out (may be NULL): depth entries, index = page. */
int  vm_video_optimize_level(vm_video *v, int lvl, float max_iter, volatile const int *run_flag,
                             int fixed_work, vm_progress *out);
/* Morph::calculate_halfway_parametrization, morph.cu:150-168.  per_page (may be NULL): for
 * every level with images (finest first) its depth entries. */
int  vm_video_solve(vm_video *v, float max_iter, float max_iter_drop_factor,
                    const vm_video_constraint *c, int n, volatile const int *run_flag,
                    int fixed_work, vm_progress *per_page);

/* ---- error view: where the match is poor, and how good the solve is -------- */
/* The reference's UI has an "Error Image" entry next to "Halfway Image" whose slot only sets a flag
 * (UI/MdiEditor.cpp:1928-1933): the image is never computed.  Here it is.  Per pixel of a level (or of one page of a
 * video level) the terms of the energy the sweep minimises, morph.cu:730-761 -- float32 planes, DESIGN.md 3.8:
 *   e_ssim = (w_ssim * (1 - value)) * inv_wh
 *   e_tps  =  w_tps * (0.5 * (v.x * tps_b.x + v.y * tps_b.y))
 *   e_ui   =  ui_axy > 0 ? (w_ui * ((ui_b.x^2 + ui_b.y^2) / (4 * ui_axy))) * inv_wh : 0
 *   e_temp =  flag ? (((w_temp * (|v.x - ref.x| + |v.y - ref.y|)) * temp_mask) * factor_d) * inv_wh : 0
 *   e_all  = ((e_ssim + e_tps) + e_ui) + e_temp
 * from the arrays vm_level_get_field returns at that moment and the context's vm_kern_params; flag is what the sweep
 * of that page runs with (false for a vm_pyr and for the page a video level solves first).  The same bits in every
 * math mode.  `what` picks a plane; the totals are the five sums in that order, doubles folded in one fixed order
 * that the level's geometry decides: the same bits from run to run, on any context, alone or in a batch.
 * VM_E_STATE when the level holds no initialised state (the coarsest level; before vm_init_level; after
 * vm_level_clear), VM_E_INVALID for a bad what / level / page / size or a NULL output.  The level is not changed. */
enum { VM_ERR_SSIM = 0, VM_ERR_TPS, VM_ERR_UI, VM_ERR_TEMP, VM_ERR_ALL };
/* the five totals of one level (UI/MdiEditor.cpp:1928-1933; morph.cu:730-761) */
int  vm_level_energy(vm_pyr *pyr, int lvl, double *out5);
/* the same for level `lvl` of n pyramids of one context and one geometry in ONE launch (UI/MdiEditor.cpp:1928-1933;
 * morph.cu:730-761); out5n: n x 5, pair-major; each pair's bits are those of its own vm_level_energy */
int  vm_level_energy_batch(vm_pyr **pyrs, int n, int lvl, double *out5n);
/* one plane to the host, h rows of w floats, pitch in floats, 0 = tight (UI/MdiEditor.cpp:1928-1933; morph.cu:730-761) */
int  vm_level_error_map(vm_pyr *pyr, int lvl, int what, float *plane, int pitch);
/* the view itself (UI/MdiEditor.cpp:1928-1933; morph.cu:730-761): plane `what` sampled to w0 x h0 with the sampling of
 * vm_upscale_result (MatchingThread.cpp:103-136; the plane is not rescaled by the size ratio), t = clamp(s * gain, 0, 1),
 * heat ramp r = min(3t, 1), g = clamp(3t - 1, 0, 1), b = clamp(3t - 2, 0, 1), each byte (uint8)(c * 255 + 0.5);
 * rgb: h0 rows of w0 RGB8 pixels, pitch in bytes (0 = tight), bytes beyond a row's 3 w0 are not written */
int  vm_level_error_image(vm_pyr *pyr, int lvl, int what, float gain, int w0, int h0, uint8_t *rgb, int pitch_bytes);
/* the same three for one page of a video level (UI/MdiEditor.cpp:1928-1933; morph.cu:730-761, the temporal term :752-759) */
int  vm_video_energy(vm_video *v, int lvl, int page, double *out5);
int  vm_video_error_map(vm_video *v, int lvl, int page, int what, float *plane, int pitch);
int  vm_video_error_image(vm_video *v, int lvl, int page, int what, float gain, int w0, int h0, uint8_t *rgb,
                          int pitch_bytes);

/* ---- compositor ---------------------------------------------------------- */
typedef struct vm_frame vm_frame;
/* device-resident inputs of one output frame: the two Poisson-extended RGBA8
 * canvases (w+2ex)x(h+2ex) (Pyramid::_extends1/_extends2, Pyramid.h:44-45),
 * the full-resolution halfway field and quadratic path (Pyramid::_vector,
 * _qpath).  Replaces the per-frame cudaMallocArray/H2D uploads of
 * RenderWidget::RenderStage2, UI/RenderWidget.cpp:229-266.  qpath may be NULL
 * (zero path: CQuadraticPath is disabled in the reference app). */
int  vm_frame_create(vm_ctx *ctx, int w, int h, int ex, vm_frame **out);
void vm_frame_destroy(vm_frame *f);
int  vm_frame_upload(vm_frame *f, const uint8_t *ext0_rgba, const uint8_t *ext1_rgba,
                     const float *v_xy, const float *qpath_xy);
/* the same from the two RGB8 frames themselves (h rows of pitch_bytes, 0 = tight): the canvases are built on the device as
 * Pyramid::build builds them, Algorithm/pyramid.cu:186-200 (frame + zero alpha plane pasted at (ex, ex) into a canvas of
 * (255, 255, 255, 255)); v and the quadratic path stay what they are.  12 MB over the link per 1080p pair instead of 27. */
int  vm_frame_upload_rgb(vm_frame *f, const uint8_t *rgb0, const uint8_t *rgb1, int pitch_bytes);
int  vm_frame_download_ext(vm_frame *f, int side, uint8_t *ext_rgba);
/* take v straight from a solved pyramid level (device to device, with the
 * update_result upscale) */
int  vm_frame_set_v_from_level(vm_frame *f, vm_pyr *pyr, int lvl);
/* Page-lock / release a host buffer the caller uploads frames from (the reference re-uploads 108 MB of float4
 * canvases per rendered frame from pageable memory, UI/RenderWidget.cpp:229-266; here 27 MB of RGBA8 per frame
 * pair, once): vm_frame_upload from a registered buffer runs at the link's rate.  Optional. */
int  vm_host_register(void *ptr, uint64_t bytes);
int  vm_host_unregister(void *ptr);
/* ... and frame `frame` of vm_video_result (above), computed on the device */
int  vm_frame_set_v_from_video(vm_frame *f, vm_video *v, int lvl, int frame);
/* The render calls -- every vm_render_* from here to the viewports over a shutter, the vm_frame_render_viewport_filtered*
 * and the vm_frame_render_multiband* among them, and each one's _dev twin -- refuse in
 * one order: the handle (VM_E_INVALID); a NULL output of a call that downloads (VM_E_INVALID); the arguments -- viewport,
 * samples, samples * nx * ny, bands, ease, filter, color_from (VM_E_INVALID); the frame's state -- no schedule, then no layers
 * (VM_E_STATE); a pitch below the row (VM_E_INVALID).  Of two faults at once the earlier one answers. */
/* render_halfway_image, Algorithm/render.cu:62-96 (UI/RenderWidget.h:52-57);
 * rgb_out: h rows of w RGB8 pixels, pitch in bytes (0 = tight) */
int  vm_render_halfway(vm_frame *f, float color_fa, float geo_fa, int color_from,
                       uint8_t *rgb_out, int pitch_bytes);
/* same, output left on the device (for timing / chaining) */
int  vm_render_halfway_dev(vm_frame *f, float color_fa, float geo_fa, int color_from,
                           float *elapsed_ms);
/* What the fixed point of vm_render_halfway (kernel_render_halfway_image, Algorithm/render.cu:16-60; the per-frame
 * call of UI/RenderWidget.cpp:229-266) knows besides a colour.  After its 20 rounds an output pixel holds (px, py), the
 * blended v and, if the frame has a path, u -- the renderer's float32 expressions in the renderer's order:
 *   map0 = (px - v.x, py - v.y), map1 = (px + v.x, py + v.y): where the pixel samples image 0 and image 1, in image
 *     pixels (pixel centre i is i; the renderer adds ex + 0.5f to these).  At geo_fa = 0 map1 is the forward map image
 *     0 -> image 1, at geo_fa = 1 map0 the backward map.  Tight (h, w, 2) floats each;
 *   resid = fmaxf(|px20 - px19|, |py20 - py19|): the move of the last round, tight (h, w) floats;
 *   flags, tight (h, w) bytes: bit 0 set when 0 <= map0.x <= w - 1 && 0 <= map0.y <= h - 1, bit 1 the same for map1 (a NaN
 *     coordinate fails the comparisons).
 * Any output may be NULL, not all four (VM_E_INVALID).  The frame is not changed. */
int  vm_frame_sampling_maps(vm_frame *f, float geo_fa, float *map0_xy, float *map1_xy, float *resid, uint8_t *flags);
/* Two w x h float32 layers of 1..4 interleaved channels (h rows of pitch_floats, 0 = tight) -- a matte, a depth or UV pass,
 * a float plate -- kept on the device beside the canvases render.cu:16-60 samples (UI/RenderWidget.cpp:229-266 uploads
 * only those).  Storage is allocated on the first upload; uploading again replaces the layers and may change `channels`. */
int  vm_frame_upload_layers(vm_frame *f, int channels, const float *layer0, const float *layer1, int pitch_floats);
/* The layers through the morph (the chain of render.cu:16-60, UI/RenderWidget.cpp:229-266): layer k is sampled at
 * (mapk.x + 0.5f, mapk.y + 0.5f) with the field taps' bilinear expression, per channel (1-a)(1-b) t00 + a(1-b) t10 +
 * (1-a)b t01 + ab t11 from left to right, indices clamped to the layer: the edge texel repeats (flags of
 * vm_frame_sampling_maps tell where) unless the layers have been extended (vm_frame_extend_layers, below).  color_from 0: c0, 2: c1, 1: c0 * (1 - color_fa) + c1 * color_fa in float32.
 * out: (h, w, channels) floats, pitch in floats (0 = tight).  VM_E_STATE on a frame that holds no layers. */
int  vm_render_layers(vm_frame *f, float color_fa, float geo_fa, int color_from, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_layers_dev(vm_frame *f, float color_fa, float geo_fa, int color_from, float *elapsed_ms);
/* ---- the layers past the image edge -----------------------------------------
 * The layers extended as the canvases are (PoissonExt.cpp:49-362): per side a (ch, cw, channels) float32 canvas, cw = w +
 * 2 ex, ch = h + 2 ex, the tight layer at (ex, ex); every cell outside the image filled by following the halfway field
 * into the OTHER side's tight layer (the RGB fill's chain; the bilinear value unrounded; a landing point outside
 * [0, w) x [0, h) leaves a hole); then the screened Poisson system of the RGB path on the image's outermost ring and the
 * cells outside it, holes starting from 0, per group of up to three channels through the solver of vm_poisson_extend_frames
 * (both sides of a group one batch; vm_set_reduction applies).  The solution is pasted as it is, neither clamped nor
 * rounded; the cells inside the ring keep their bits.  From then on EVERY layer render call of this header samples the
 * canvases at ((map + ex) + 0.5f) -- the renderer's own + ex + 0.5f -- instead of the tight layers at (map + 0.5f); flags and
 * the maps keep their meaning.  iters / rel_res: two entries per channel group ((channels + 2) / 3 groups), side 1 then side
 * 2; either may be NULL.  A group whose right-hand side is all zeros (an empty matte) extends to zeros without a solve
 * (0 iterations).  VM_E_STATE without layers or with ex == 0; VM_E_INVALID for tol <= 0 or max_it < 1; VM_E_NUMERIC for a
 * residual above tol or a right-hand side that is not finite -- the frame then renders its tight layers.  v, the path, the
 * RGB canvases and the schedule are not touched.  vm_frame_upload_layers drops the extension (extend again);
 * vm_frame_set_v_* and vm_frame_upload leave it as it is, as they leave the RGB canvases. */
int  vm_frame_extend_layers(vm_frame *f, float tol, int max_it, int *iters, float *rel_res, float *elapsed_ms);
/* the extended layer of side 1 or 2 (PoissonExt.cpp:49-362): (ch, cw, channels) floats, pitch in floats (0 = tight).
 * VM_E_STATE on a frame whose layers are not extended. */
int  vm_frame_download_layers_ext(vm_frame *f, int side, float *out, int pitch_floats);
/* back to the tight layers (the canvases of PoissonExt.cpp:49-362 stay allocated); a no-op on a frame without extension */
int  vm_frame_drop_layer_extension(vm_frame *f);
/* Diagnostic: what the extension of one side (PoissonExt.cpp:49-362) solves, before any solve -- the filled canvas
 * (ch, cw, channels) floats, `valid` (ch, cw) bytes (1: the cell holds a value, 0: a hole), the type map (ch, cw) bytes (2
 * outside the image, 1 its outermost ring, 0 inside) and the right-hand side (ch, cw, channels) floats.  Any output may be
 * NULL.  Works on buffers of its own: the frame, extended or not, is not changed.  VM_E_STATE without layers. */
int  vm_dbg_layers_prepare(vm_frame *f, int side, float *filled, uint8_t *valid, uint8_t *type, float *rhs);
/* ---- transition control: where the morph happens when ---------------------
 * The calls above take one geo_fa and one color_fa for the whole frame.  A frame may instead hold a SCHEDULE: two planes
 * of w x h float pairs (t0, t1) in the halfway domain (the domain of v), one for the geometry and one for the colour.  A
 * texel starts its transition at time t0 and ends it at t1.  For a call at time t with ease e every texel's rate is, in
 * float32 and in this order (the division correctly rounded):
 *   d = t1 - t0;  s = d > 0 ? fminf(fmaxf((t - t0) / d, 0), 1) : (t >= t0 ? 1 : 0)
 *   rate = e == VM_EASE_SMOOTH ? (s * s) * (3 - 2 * s) : s
 * which gives the rate planes G (geometry) and K (colour); t is not clamped.  Both are sampled at the tap positions of
 * the chain of kernel_render_halfway_image (Algorithm/render.cu:16-60) with the field taps' index and clamp arithmetic, in
 * lerp form: r0 = t00 + a (t10 - t00), r1 = t01 + a (t11 - t01), r = r0 + b (r1 - r0) (a constant plane gives its value
 * exactly).  The chain is the renderer's with g = tapr(G, p) in the place of geo_fa, taken anew (undamped) at every p:
 *   p = q, V = tap(v, p), U = tap(u, p), g = tapr(G, p);  20 rounds: s1 = 2 g - 1, s2 = 4 g - 4 g g,
 *   p = (q - s1 V) - s2 U, V = 0.8 tap(v, p) + (1 - 0.8) V, U likewise, g = tapr(G, p);  then k = tapr(K, p) in the
 *   place of color_fa.
 * The geometric rate belongs to the halfway-domain point p the chain looks for, not to the output pixel: uniform frames
 * mixed by a matte on the host tear at every rate gradient, this does not.  With the schedule (0, 1) everywhere and
 * VM_EASE_LINEAR, G is exactly t for t in [0, 1] and every call below gives the bits of its uniform counterpart at
 * geo_fa = color_fa = t.  A discontinuous schedule can keep the chain from settling (a hard step t1 == t0 across a lead
 * ramp: a resid of several pixels at the seam): that is the caller's business, resid of vm_frame_transition_maps reports it. */
#define VM_EASE_LINEAR 0
#define VM_EASE_SMOOTH 1
/* The schedule (render.cu:16-60; stored beside what UI/RenderWidget.cpp:229-266 uploads per frame): (h, w, 2) floats
 * each, h rows of pitch_floats (0 = tight).  Either plane may be NULL: uniform (0, 1); both NULL: VM_E_INVALID.  Kept on
 * the device beside the layers; a new upload replaces it. */
int  vm_frame_upload_schedule(vm_frame *f, const float *geo_t0t1, const float *color_t0t1, int pitch_floats);
/* the frame holds no schedule from here on (render.cu:16-60, UI/RenderWidget.cpp:229-266: the calls below answer VM_E_STATE) */
int  vm_frame_clear_schedule(vm_frame *f);
/* vm_render_halfway under the schedule at time t (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the
 * Poisson-extended canvases with the renderer's tail (+ ex + 0.5f, the blend c0 * (1 - k) + c1 * k for color_from 1, + 0.5
 * in double, truncation).  rgb_out: h rows of w RGB8 pixels, pitch in bytes (0 = tight).  VM_E_STATE without a schedule;
 * VM_E_INVALID for an ease other than VM_EASE_LINEAR / VM_EASE_SMOOTH, a color_from outside 0..2, a pitch below the row,
 * a NULL output.  The frame's v, path, canvases and layers are not changed by any of the calls of this section. */
int  vm_render_transition(vm_frame *f, float t, int ease, int color_from, uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_transition_dev(vm_frame *f, float t, int ease, int color_from, float *elapsed_ms);
/* vm_render_layers under the schedule (render.cu:16-60, UI/RenderWidget.cpp:229-266): the layers of vm_frame_upload_layers
 * through the same chain, blended with k.  out: (h, w, channels) floats, pitch in floats (0 = tight).  VM_E_STATE without a
 * schedule or without layers. */
int  vm_render_transition_layers(vm_frame *f, float t, int ease, int color_from, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_transition_layers_dev(vm_frame *f, float t, int ease, int color_from, float *elapsed_ms);
/* vm_frame_sampling_maps under the schedule (render.cu:16-60, UI/RenderWidget.cpp:229-266): its four outputs, and
 * rates_gk, tight (h, w, 2) floats: (g, k) as they stand after round 20.  Any output may be NULL, not all five
 * (VM_E_INVALID). */
int  vm_frame_transition_maps(vm_frame *f, float t, int ease, float *map0_xy, float *map1_xy, float *resid, uint8_t *flags,
                              float *rates_gk);
/* ---- points and motion vectors through the morph ---------------------------
 * The maps above go from the pixel grid of one output frame to image 0 and image 1.  The carry calls take any position of
 * an output frame and return that position at other times of the morph: markers, roto shapes and mesh vertices drawn on
 * every frame, a motion-vector pass, the gap a constraint is left with.  For a start point q = (x, y) of the output frame
 * at geo_fa = from_fa (pixel centre i is i, as in the maps), in float32, in this order, without contraction:
 *   the chain of kernel_render_halfway_image (Algorithm/render.cu:16-60; UI/RenderWidget.cpp:229-266) from q: p = q,
 *   V = tap(v, p), U = tap(u, p); 20 rounds: p = (q - s1 V) - s2 U, V = 0.8 tap(v, p) + (1 - 0.8) V, U likewise (U = 0
 *   without a path), with s1 = 2 from_fa - 1, s2 = 4 from_fa - 4 from_fa from_fa.  After round 20:
 *   halfway = (px, py);  pos0 = (px - V.x, py - V.y);  pos1 = (px + V.x, py + V.y): the point in the halfway domain, in
 *     image 0 and in image 1;
 *   resid = fmaxf(|px20 - px19|, |py20 - py19|);  flags: bit 0 set when pos0 is inside the image, bit 1 when pos1 is (the
 *     comparisons of vm_frame_sampling_maps);
 *   for every to-time g = to_fa[k]:  s1 = 2 g - 1;  s2 = 4 g - 4 g g;
 *     out[k] = ((px + s1 V.x) + s2 U.x, (py + s1 V.y) + s2 U.y)      (the s2 term is added without a path too, U = 0).
 * Image 0 is time 0 and image 1 is time 1: "from image 0", "from image 1" and "from a rendered frame" are one call with
 * another from-time.  Neither from_fa nor the to-times are clamped.  Under a schedule (the _transition forms; the section
 * above) the chain runs with g = tapr(G, p), G the geometry plane ramped at t_from, and the rate of a to-time t_k is the
 * same tap at p of round 20 -- the four schedule texels and fractions of tap_at(px + 0.5f, py + 0.5f) -- with the ramp
 * taken at t_k: g_k = lerp(ramp(s00, t_k), ramp(s10, t_k), ramp(s01, t_k), ramp(s11, t_k)); then s1, s2 and out[k] as
 * above.  The colour plane plays no part.  With the schedule (0, 1), VM_EASE_LINEAR and all times in [0, 1] every output
 * has the bits of the uniform call.  The property that a point carried from s to t and back returns holds where the
 * field is invertible and the chain has settled (resid).
 * Outputs: out_xy (nt, n, 2) floats; halfway_xy, pos0_xy, pos1_xy (n, 2) floats; resid n floats; flags n bytes.  Any output
 * may be NULL, not all of them; elapsed_ms (the launch, by events) may be NULL.  The calls refuse in the order of the
 * render calls: the handle; every output NULL, a NULL pts_xy or a NULL times array; the arguments -- n outside 1..2^26, nt outside
 * 1..64 (the dense calls: 1..16), a from-time or a to-time that is not finite, an ease outside the two (all
 * VM_E_INVALID); the state -- no schedule for the _transition forms (VM_E_STATE).  The points are not scanned: a NaN, an
 * infinite or a huge coordinate goes through the chain's clamps like a NaN of the field and comes out as the statement
 * says.  The frame is not changed. */
int  vm_frame_carry_points(vm_frame *f, float from_fa, const float *pts_xy, int n, const float *to_fa, int nt,
                           float *out_xy, float *halfway_xy, float *pos0_xy, float *pos1_xy, float *resid, uint8_t *flags,
                           float *elapsed_ms);
/* same under the frame's schedule (render.cu:16-60, UI/RenderWidget.cpp:229-266): the from-time and the to-times are
 * times of the schedule */
int  vm_frame_carry_points_transition(vm_frame *f, float t_from, int ease, const float *pts_xy, int n, const float *t_to,
                                      int nt, float *out_xy, float *halfway_xy, float *pos0_xy, float *pos1_xy, float *resid,
                                      uint8_t *flags, float *elapsed_ms);
/* The motion maps (render.cu:16-60, UI/RenderWidget.cpp:229-266): the carry call from the w x h pixel centres of the
 * output frame at from_fa -- "output pixel at time s to its position at time t", a motion-vector pass once the pixel's own
 * position is subtracted.  out_xy (nt, h, w, 2) floats, resid (h, w) floats, flags (h, w) bytes; any may be NULL, not all
 * three.  nt in 1..16.  For the to-times {0, 1} out is map0 / map1 of vm_frame_sampling_maps at geo_fa = from_fa. */
int  vm_frame_motion_maps(vm_frame *f, float from_fa, const float *to_fa, int nt, float *out_xy, float *resid, uint8_t *flags);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), all three outputs left on the device (for timing) */
int  vm_frame_motion_maps_dev(vm_frame *f, float from_fa, const float *to_fa, int nt, float *elapsed_ms);
/* the motion maps under the frame's schedule (render.cu:16-60, UI/RenderWidget.cpp:229-266) */
int  vm_frame_transition_motion_maps(vm_frame *f, float t_from, int ease, const float *t_to, int nt, float *out_xy,
                                     float *resid, uint8_t *flags);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), all three outputs left on the device (for timing) */
int  vm_frame_transition_motion_maps_dev(vm_frame *f, float t_from, int ease, const float *t_to, int nt, float *elapsed_ms);
/* ---- motion blur: the morph integrated over a shutter ----------------------
 * A frame rendered at one instant is sharp however fast its content moves; a sequence of them strobes.  A shutter call
 * walks the chain of kernel_render_halfway_image (Algorithm/render.cu:16-60) at N = samples times per output pixel, in one
 * launch, and returns the mean of the samples' colours.  In float32, in this order (the divisions correctly rounded), for
 * s = 0 .. N - 1:
 *   f   = ((float)s + 0.5f) / (float)N
 *   t_s = fminf(fmaxf(geo_open + (geo_close - geo_open) * f, 0), 1)
 *   c_s = the colour of the uniform call at geo_fa = t_s, before its rounding: the taps at (map0, map1)_s blended by
 *         color_from with the call's one color_fa (the colour fraction stays fixed over the exposure: a dissolve is not motion)
 *   acc = acc + c_s                              (acc starts at +0)
 * and the result is acc / (float)N.  The times are clamped, so a shutter open across t = 0 or t = 1 holds still outside
 * the morph; geo_close < geo_open is legal.  With samples = 1 and geo_open == geo_close == g in [0, 1] a call gives the bits
 * of its uniform counterpart at geo_fa = g.  Every call of this section answers VM_E_INVALID for samples outside 1..64, a
 * color_from outside 0..2, a pitch below the row or a NULL output, and changes nothing of the frame (v, path, canvases,
 * layers, schedule).  The schedule of the section above is not consulted (the section below does). */
/* vm_render_halfway over the shutter (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the Poisson-extended
 * canvases, (uint8)((double)(acc / (float)N) + 0.5) per channel.  rgb_out: h rows of w RGB8 pixels, pitch in bytes (0 = tight). */
int  vm_render_shutter(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples, int color_from,
                       uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_shutter_dev(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples, int color_from,
                           float *elapsed_ms);
/* vm_render_layers over the shutter (render.cu:16-60, UI/RenderWidget.cpp:229-266): the layers of vm_frame_upload_layers
 * through the same sample times, so that a matte blurs exactly as its plate does.  out: (h, w, channels) floats, pitch in
 * floats (0 = tight).  VM_E_STATE on a frame that holds no layers. */
int  vm_render_shutter_layers(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples, int color_from,
                              float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_shutter_layers_dev(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples, int color_from,
                                  float *elapsed_ms);
/* ---- motion blur under a transition schedule ------------------------------
 * The two sections above together: the shutter of a frame that holds a schedule.  The geometry schedule is ramped anew at
 * every sample time, the colour schedule once, at t_color (the colour time stays fixed over the exposure: a dissolve is
 * not motion).  In float32, in this order (the divisions correctly rounded), with ramp, tapr and the chain as the
 * transition section states them, N = samples:
 *   K   = ramp(schedule_colour, t_color, ease)
 *   for s = 0 .. N - 1:
 *     f   = ((float)s + 0.5f) / (float)N
 *     t_s = t_open + (t_close - t_open) * f      (not clamped: ramp clamps per texel, as for vm_render_transition's t)
 *     G_s = ramp(schedule_geometry, t_s, ease)
 *     p_s, V_s = the chain under G_s;  k_s = tapr(K, p_s)
 *     c_s = the colour of vm_render_transition / vm_render_transition_layers on them before its rounding, blended by
 *           color_from with k_s
 *     acc = acc + c_s                            (acc starts at +0)
 * and the result is acc / (float)N.  With samples = 1 and t_open == t_close == t_color == t a call gives the bits of its
 * transition counterpart at t; with the schedule (0, 1) on both planes and VM_EASE_LINEAR it gives the bits of its shutter
 * counterpart at color_fa = t_color in [0, 1], geo_open = t_open, geo_close = t_close.  t_close < t_open is legal.  Every
 * call of this section answers VM_E_INVALID for samples outside 1..64, an ease other than VM_EASE_LINEAR /
 * VM_EASE_SMOOTH, a color_from outside 0..2, a pitch below the row or a NULL output, and VM_E_STATE on a frame without a
 * schedule.  The frame's v, path, canvases, layers and schedule are not changed; no device memory depends on samples. */
/* vm_render_transition over the shutter (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the Poisson-extended
 * canvases, (uint8)((double)(acc / (float)N) + 0.5) per channel.  rgb_out: h rows of w RGB8 pixels, pitch in bytes (0 = tight). */
int  vm_render_transition_shutter(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease, int color_from,
                                  uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_transition_shutter_dev(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                      int color_from, float *elapsed_ms);
/* vm_render_transition_layers over the shutter (render.cu:16-60, UI/RenderWidget.cpp:229-266): the layers of
 * vm_frame_upload_layers through the same sample times and rates, so that a matte stays in step with its plate.  out:
 * (h, w, channels) floats, pitch in floats (0 = tight).  VM_E_STATE on a frame that holds no layers. */
int  vm_render_transition_shutter_layers(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                         int color_from, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_transition_shutter_layers_dev(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                             int color_from, float *elapsed_ms);
/* ---- viewports: any window of the morph at any size, supersampled ----------
 * The calls above render the w x h grid of the field, one chain per pixel from the pixel's centre.  A viewport call lays an
 * out_w x out_h grid freely over the halfway domain -- a zoom, a pan, a proxy, a delivery size, overscan into the
 * Poisson-extended canvases -- and starts the chain of kernel_render_halfway_image (Algorithm/render.cu:16-60) from a
 * regular nx x ny grid of sub-sample points inside every output pixel, in one launch, and returns the mean of the samples'
 * colours.  Coordinates are pixel-EDGE: field pixel i covers [i, i + 1), its centre is i + 0.5. */
typedef struct vm_viewport {
    float x0, y0;           /* top-left corner of the output in field coordinates */
    float step_x, step_y;   /* field pixels per output pixel (1 = native, 0.5 = 2x enlargement, 2 = half size) */
    int   out_w, out_h;     /* output size, 1..32768 each */
    int   nx, ny;           /* sub-samples per output pixel, a regular nx x ny grid; 1 <= nx * ny <= 64 */
} vm_viewport;
/* In float32, in this order (the divisions correctly rounded), for output pixel (X, Y) and sub-sample s = j * nx + i
 * (i fastest, s = 0 .. N - 1, N = nx * ny):
 *   fx = ((float)i + 0.5f) / (float)nx             fy = ((float)j + 0.5f) / (float)ny
 *   qx = (x0 + ((float)X + fx) * step_x) - 0.5f    qy = (y0 + ((float)Y + fy) * step_y) - 0.5f
 *   (p, V)_s = the chain as vm_frame_sampling_maps states it, with q = (qx, qy) in the place of the pixel, at the call's
 *              geo_fa (not clamped)
 *   c_s = the colour of the uniform call on (map0, map1)_s = (p - V, p + V) before its rounding, blended by color_from
 *         with the call's color_fa
 *   acc = acc + c_s                                (acc starts at +0)
 * and the result is acc / (float)N.  The field, the path, the canvases and the layers are read outside [0, w) x [0, h) as
 * the chain reads them wherever a warp leaves the image (clamped taps), so a viewport may lie partly or wholly outside the
 * field.  {0, 0, 1, 1, w, h, 1, 1} gives the bits of the uniform call; integer x0, y0 with step 1 and one sample give the
 * corresponding slice of it; with a zero field and no path {0, 0, 2, 2, w / 2, h / 2, 2, 2} reads exactly the four texels
 * of every 2 x 2 block: an exact box reduction.  Every call of this section answers VM_E_INVALID for a NULL viewport or
 * output, a non-finite x0, y0 or step, a step that is not > 0, out_w or out_h outside 1..32768, nx < 1, ny < 1 or
 * nx * ny > 64, a color_from outside 0..2 or a pitch below the output's row, and changes nothing of the frame (v, path,
 * canvases, layers, schedule); no device memory depends on nx * ny.  Not in this section, deliberately: viewport sampling
 * maps.  The schedule is not consulted here (the section after this one does). */
/* vm_render_halfway through a viewport (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the Poisson-extended
 * canvases, (uint8)((double)(acc / (float)N) + 0.5) per channel.  rgb_out: out_h rows of out_w RGB8 pixels, pitch in bytes
 * (0 = tight). */
int  vm_render_viewport(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from, uint8_t *rgb_out,
                        int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_viewport_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from, float *elapsed_ms);
/* vm_render_layers through a viewport (render.cu:16-60, UI/RenderWidget.cpp:229-266): the layers of vm_frame_upload_layers
 * from the same sub-sample points, so that a matte is filtered exactly as its plate is.  out: (out_h, out_w, channels)
 * floats, pitch in floats (0 = tight).  VM_E_STATE on a frame that holds no layers. */
int  vm_render_viewport_layers(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from, float *out,
                               int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_viewport_layers_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                   float *elapsed_ms);
/* ---- viewports through a cubic filter ----------
 * A viewport call taps its colour, at the end of its chain, with four texels: a 2.5x zoom magnifies the plate through a
 * bilinear kernel, which is soft and shows its diamond pattern along edges (supersampling does not help: under
 * magnification it averages more bilinear values).  The calls of this section take the viewport section's arguments,
 * outputs and refusals, and a filter for the taps that read picture content -- a canvas, a layer: */
#define VM_FILTER_BILINEAR    0
#define VM_FILTER_CATMULL_ROM 1   /* B = 0,   C = 1/2: interpolating */
#define VM_FILTER_MITCHELL    2   /* B = 1/3, C = 1/3 */
#define VM_FILTER_BSPLINE     3   /* B = 1,   C = 0: never overshoots, blurs */
/* Everything is as the viewport section states it: q, the chain, (map0, map1)_s = (p - V, p + V), the blend by color_from /
 * color_fa, acc = acc + c_s in sample order, acc / (float)N.  The one exception is the tap that reads a canvas or a layer;
 * the chain's own taps of the field stay bilinear (it taps a smooth vector field, and its bits are the reference's).
 * A cubic tap reads a W x H image at (x, y).  These are the coordinates that the bilinear tap takes: the canvases'
 * + ex + 0.5f, the layers' (+ lexf) + 0.5f.  It works in float32, without contraction, in this order:
 *   xb = x - 0.5f;  fi = floorf(xb);  a = xb - fi;  fi = fminf(fmaxf(fi, -2.0f), (float)W + 1.0f);  i = (int)fi
 *   columns  c_k = clamp(i + k, 0, W - 1),  k = -1, 0, 1, 2                 (rows r_m from y, b, H likewise)
 *   inner(d) = ((p3 * d + p2) * d) * d + p0            outer(d) = ((q3 * d + q2) * d + q1) * d + q0
 *   wx_-1 = outer(1.0f + a)   wx_0 = inner(a)   wx_1 = inner(1.0f - a)   wx_2 = outer(2.0f - a)     (wy from b likewise)
 *   row_m = ((wx_-1 * t(c_-1, r_m) + wx_0 * t(c_0, r_m)) + wx_1 * t(c_1, r_m)) + wx_2 * t(c_2, r_m)
 *   value = ((wy_-1 * row_-1 + wy_0 * row_0) + wy_1 * row_1) + wy_2 * row_2
 * The value is per channel, and uchar -> float is exact.  No tap reads outside the image whatever x is -- NaN, +-inf, 1e30:
 * the float clamp before the conversion guarantees it.  The coefficients are one host table per filter, each (float)(n / d)
 * with n, d doubles:
 *   filter        p3    p2    p0    q3     q2    q1     q0
 *   Catmull-Rom   3/2   -5/2  1     -1/2   5/2   -4     2
 *   Mitchell      7/6   -2    8/9   -7/18  2     -10/3  16/9
 *   B-spline      1/2   -1    2/3   -1/6   1     -2     4/3
 * Cubic filters overshoot: a 0 / 255 step tapped at a = 0.25 gives 272.93 and -17.93 under Catmull-Rom, 260.98 and -5.98
 * under Mitchell.  The RGB8 result is (uint8)((double)fminf(fmaxf(acc / (float)N, 0.0f), 255.0f) + 0.5); samples are not
 * clamped one by one.  Layers are returned UNCLAMPED: a matte may leave [0, 1]; that is the filter's answer, and the caller
 * decides what to do with it.  Extended layers (vm_frame_extend_layers) are tapped on their extended grid, as every layer
 * call taps them.  VM_FILTER_BILINEAR is the viewport call itself, bit for bit (the same kernel).  Every call of this
 * section answers VM_E_INVALID for whatever the viewport section refuses and for a filter outside 0..3, VM_E_STATE for a
 * layer call on a frame without layers, and leaves the frame (v, path, canvases, layers, schedule) unchanged after a refusal
 * as after a render.  Not in this section, deliberately: filtered forms of the shutter, transition and viewport-shutter
 * families (they take this tail as a choice later), filtered sampling maps, any change to the chain's own taps, and a
 * prefilter for the B-spline (which therefore smooths: it does not interpolate). */
/* vm_render_viewport through a filter (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the Poisson-extended
 * canvases, clamped to [0, 255] before the rounding.  rgb_out: out_h rows of out_w RGB8 pixels, pitch in bytes (0 = tight). */
int  vm_frame_render_viewport_filtered(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                       int color_from, uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_frame_render_viewport_filtered_dev(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                           int color_from, float *elapsed_ms);
/* vm_render_viewport_layers through a filter (render.cu:16-60, UI/RenderWidget.cpp:229-266): the layers of
 * vm_frame_upload_layers, unclamped.  out: (out_h, out_w, channels) floats, pitch in floats (0 = tight).  VM_E_STATE on a
 * frame that holds no layers. */
int  vm_frame_render_viewport_filtered_layers(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                              int color_from, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_frame_render_viewport_filtered_layers_dev(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                                  int color_from, float *elapsed_ms);
/* ---- multiband blending: the two plates blended band by band ----------------
 * Every render call above blends the two warped plates under ONE per-pixel weight, c0 * (1 - k) + c1 * k: a dissolve around
 * color_fa = 0.5 shows both plates' fine detail at once wherever the correspondence is a pixel off, and the colour seam of a
 * wipe is as wide as the schedule's ramp at every frequency.  The calls of this section are the multiresolution spline of
 * Burt and Adelson (1983) on the renderer's chain (kernel_render_halfway_image, Algorithm/render.cu:16-60;
 * UI/RenderWidget.cpp:229-266): the plates c0, c1 -- exactly what the uniform and the transition calls form before they
 * blend, RGB from the extended canvases or the layers of vm_frame_upload_layers, tight or extended -- and the colour weight
 * A (color_fa everywhere, or the per-pixel k of the schedule) are reduced L times; band l of both plates is blended under
 * the weight of level l, sharpened about 0.5 by sharp[l], and the bands are summed from the coarsest up.  In float32,
 * without contraction, in this order (fold reflects without repeating the edge sample: -1 -> 1, n -> n - 2):
 *   reduce, n -> (n + 1) / 2, along x and then along y, t(d) the sample at fold(2 i + d, n):
 *     (0.0625f * (t(-2) + t(2)) + 0.25f * (t(-1) + t(1))) + 0.375f * t(0)
 *   expand, m -> n, along x and then along y, i = o / 2, t(d) the sample at fold(i + d, m):
 *     o even: 0.125f * (t(-1) + t(1)) + 0.75f * t(0)        o odd: 0.5f * (t(0) + t(1))
 *   G0, G1, M: c0, c1, A reduced 0..L times;  for l = L down to 0:
 *     m = fminf(fmaxf(0.5f + (M[l] - 0.5f) * sharp[l], 0), 1)
 *     b0, b1 = G0[l], G1[l] at l == L, else G0[l] - expand(G0[l + 1]), G1[l] - expand(G1[l + 1])
 *     B = b0 * (1 - m) + b1 * m;   R = B at l == L, else expand(R) + B
 * Layer calls return R as it is, neither clamped nor rounded; RGB8 calls (uint8)((double)fminf(fmaxf(R, 0), 255) + 0.5): a
 * sharpened band can overshoot, and a NaN becomes 0.  With sharp = 1 everywhere this is the Burt-Adelson spline with mask A;
 * with sharp[l] > 1 band l crosses over in the middle 1 / sharp[l] of the transition, so that detail stays single-exposed
 * except near the midpoint.  A weight of exactly 0 (or 1) gives m = 0 (or 1) on every band: the call reconstructs c0 (c1).
 * There is no color_from: the calls are the blend.  They refuse in the render calls' order, the arguments being: bands NULL,
 * levels outside 1..VM_MULTIBAND_MAX_LEVELS, a coarsest level below 2 in either dimension, a sharp entry that is not finite or
 * below 1, an ease other than the two known (VM_E_INVALID each).  The pyramids are scratch of the frame, allocated on first
 * use and freed with it; v, the path, the canvases, the layers and the schedule are not changed.  The vm_render_* names are a
 * closed table; these calls carry the vm_frame_ prefix as the filtered viewport calls do.  Not in this section, deliberately:
 * multiband forms of the viewport, shutter and filtered families, and bands blended over time. */
#define VM_MULTIBAND_MAX_LEVELS 8
typedef struct {
    int   levels;                               /* L in 1..VM_MULTIBAND_MAX_LEVELS */
    float sharp[VM_MULTIBAND_MAX_LEVELS + 1];   /* sharp[0..L] are used: band 0 the finest, band L the low-pass residual */
} vm_bands;
/* vm_render_halfway with color_from = 1, band by band (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the
 * Poisson-extended canvases.  rgb_out: h rows of w RGB8 pixels, pitch in bytes (0 = tight). */
int  vm_frame_render_multiband(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa, uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_frame_render_multiband_dev(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa, float *elapsed_ms);
/* vm_render_layers band by band (render.cu:16-60, UI/RenderWidget.cpp:229-266).  out: (h, w, channels) floats, pitch in
 * floats (0 = tight).  VM_E_STATE on a frame that holds no layers. */
int  vm_frame_render_multiband_layers(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_frame_render_multiband_layers_dev(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa, float *elapsed_ms);
/* vm_render_transition band by band (render.cu:16-60, UI/RenderWidget.cpp:229-266): the chain under the geometry schedule,
 * A the colour rate k of every output pixel.  VM_E_STATE on a frame that holds no schedule. */
int  vm_frame_render_multiband_transition(vm_frame *f, const vm_bands *bands, float t, int ease, uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_frame_render_multiband_transition_dev(vm_frame *f, const vm_bands *bands, float t, int ease, float *elapsed_ms);
/* vm_render_transition_layers band by band (render.cu:16-60, UI/RenderWidget.cpp:229-266).  VM_E_STATE on a frame that
 * holds no schedule, then on one that holds no layers. */
int  vm_frame_render_multiband_transition_layers(vm_frame *f, const vm_bands *bands, float t, int ease, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_frame_render_multiband_transition_layers_dev(vm_frame *f, const vm_bands *bands, float t, int ease, float *elapsed_ms);
/* Diagnostic: one level of what the frame's last multiband call left (the pyramids of render.cu:16-60's two plates; the
 * reference has no counterpart), for tests that pin the kernels stage by stage.  out: tight (h_l, w_l, C) floats, C = 3
 * after an RGB8 call, the layers' channels after a layer call; tight (h_l, w_l) floats for the mask.  VM_E_STATE if the frame
 * has made no multiband call; VM_E_INVALID for a NULL out, an unknown `what`, a level outside 0..L of that call, and for
 * VM_MB_OUT at level 0 after an RGB8 call (its R is the call's bytes).  VM_MB_OUT at level 0 reads the layer call's own
 * output buffer: ask before the frame's next render call. */
#define VM_MB_G0   0   /* Gaussian level of c0 */
#define VM_MB_G1   1   /* ... of c1 */
#define VM_MB_MASK 2   /* M[l], before sharpening */
#define VM_MB_OUT  3   /* R at level l, levels 1..L; level 0 too after a layers call */
int  vm_dbg_multiband_level(vm_frame *f, int what, int level, float *out);
/* ---- viewports over a shutter, uniformly and under a transition schedule ----
 * The viewport section composed with the two motion-blur sections: a viewer that zooms into a motion-blurred frame, a
 * half-size proxy of a wipe, a delivery at another size with a shutter, an overscan render of a frame that holds a
 * schedule.  Every output pixel is the mean of the chain of kernel_render_halfway_image (Algorithm/render.cu:16-60) from
 * its nx x ny sub-sample points at each of T = samples times, in one launch.  In float32, in this order (the divisions
 * correctly rounded), with N = nx * ny; time sample tau = 0 .. T - 1 is the OUTER loop, sub-sample s = j * nx + i = 0 .. N - 1
 * the INNER one, i fastest:
 *   f_tau = ((float)tau + 0.5f) / (float)T
 *   q     = (qx, qy) of the viewport section for (X, Y, i, j), unchanged
 *   uniform (vm_render_viewport_shutter*):
 *     t_tau  = fminf(fmaxf(geo_open + (geo_close - geo_open) * f_tau, 0), 1)
 *     (p, V) = the chain from q at geo_fa = t_tau
 *     c      = the colour of the uniform call on (p - V, p + V) before its rounding, blended by color_from with color_fa
 *   scheduled (vm_render_viewport_transition_shutter*):
 *     K      = ramp(schedule_colour, t_color, ease)                     once per call
 *     t_tau  = t_open + (t_close - t_open) * f_tau                      (not clamped: ramp clamps per texel)
 *     (p, V) = the chain from q under G_tau = ramp(schedule_geometry, t_tau, ease), g = tapr(G_tau, p) anew at every p
 *     k      = tapr(K, p)
 *     c      = the colour of the transition call on (p - V, p + V) before its rounding, blended by color_from with k
 *   acc = acc + c                                                       (acc starts at +0, in loop order)
 * and the result is acc / (float)(T * N).  Reads outside the field are the chain's clamped taps, as in the viewport section.
 * With samples = 1 and geo_open == geo_close == g in [0, 1] a uniform call gives the bits of its viewport counterpart at
 * geo_fa = g; with {0, 0, 1, 1, w, h, 1, 1} a call gives the bits of its shutter counterpart; with the schedule (0, 1) on both
 * planes and VM_EASE_LINEAR a scheduled call gives the bits of the uniform one at color_fa = t_color in [0, 1].  A viewport
 * under a schedule at one instant t is a scheduled call with samples = 1 and t_open == t_close == t_color == t; it has no
 * entry points of its own.  Every call of this section answers VM_E_INVALID for anything the viewport section or the
 * shutter sections refuse -- a NULL viewport or output, a non-finite x0, y0 or step, a step that is not > 0, out_w or out_h
 * outside 1..32768, nx < 1, ny < 1 or nx * ny > 64, samples outside 1..64, a color_from outside 0..2, an ease other than
 * VM_EASE_LINEAR / VM_EASE_SMOOTH (scheduled), a pitch below the output's row -- and for samples * nx * ny > 256 (a 4 x 4
 * grid at 16 times: a condition of this interface); VM_E_STATE for a scheduled call on a frame without a schedule and for a
 * layer call on a frame without layers.  The frame's v, path, canvases, layers and schedule are not changed; no device
 * memory depends on samples or nx * ny. */
/* vm_render_viewport over the shutter (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the Poisson-extended
 * canvases, (uint8)((double)(acc / (float)(T * N)) + 0.5) per channel.  rgb_out: out_h rows of out_w RGB8 pixels, pitch in
 * bytes (0 = tight). */
int  vm_render_viewport_shutter(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close, int samples,
                                int color_from, uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_viewport_shutter_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close,
                                    int samples, int color_from, float *elapsed_ms);
/* vm_render_viewport_layers over the shutter (render.cu:16-60, UI/RenderWidget.cpp:229-266): the layers of
 * vm_frame_upload_layers from the same points at the same times.  out: (out_h, out_w, channels) floats, pitch in floats
 * (0 = tight). */
int  vm_render_viewport_shutter_layers(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close,
                                       int samples, int color_from, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_viewport_shutter_layers_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close,
                                           int samples, int color_from, float *elapsed_ms);
/* vm_render_transition_shutter through a viewport (render.cu:16-60, UI/RenderWidget.cpp:229-266): RGB8 from the
 * Poisson-extended canvases under the schedule.  rgb_out: out_h rows of out_w RGB8 pixels, pitch in bytes (0 = tight). */
int  vm_render_viewport_transition_shutter(vm_frame *f, const vm_viewport *vp, float t_open, float t_close, int samples,
                                           float t_color, int ease, int color_from, uint8_t *rgb_out, int pitch_bytes);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_viewport_transition_shutter_dev(vm_frame *f, const vm_viewport *vp, float t_open, float t_close, int samples,
                                               float t_color, int ease, int color_from, float *elapsed_ms);
/* vm_render_transition_shutter_layers through a viewport (render.cu:16-60, UI/RenderWidget.cpp:229-266): the layers of
 * vm_frame_upload_layers under the same rates.  out: (out_h, out_w, channels) floats, pitch in floats (0 = tight). */
int  vm_render_viewport_transition_shutter_layers(vm_frame *f, const vm_viewport *vp, float t_open, float t_close, int samples,
                                                  float t_color, int ease, int color_from, float *out, int pitch_floats);
/* same (render.cu:16-60, UI/RenderWidget.cpp:229-266), output left on the device (for timing) */
int  vm_render_viewport_transition_shutter_layers_dev(vm_frame *f, const vm_viewport *vp, float t_open, float t_close,
                                                      int samples, float t_color, int ease, int color_from, float *elapsed_ms);
/* CPoissonExt::prepare + poissonExtend for one side (1 or 2) of the frame,
 * Algorithm/PoissonExt.cpp:49-362, on the device-resident canvases: matrix-free
 * multigrid-preconditioned CG instead of MKL DSS.  iters/rel_res may be NULL. */
int  vm_poisson_extend(vm_frame *f, int side, float tol, int max_it,
                       int *iters, float *rel_res, float *elapsed_ms);
/* The body of CPoissonExt::run's frame loop (Algorithm/PoissonExt.cpp:24-36: prepare + poissonExtend of
 * side 1, then of side 2) for n frames of one context and one size AT ONCE: side 1 samples the original
 * image 2 and side 2 the original image 1 (the copies taken at :26-27, here at vm_frame_upload), so the
 * 2 n systems are independent and share every kernel launch (blockIdx.z = system).  Same results per system
 * as vm_poisson_extend.  iters / rel_res (may be NULL): 2 n entries, [2 i] = side 1 of frames[i], [2 i + 1] =
 * side 2.  n <= 32. */
int  vm_poisson_extend_frames(vm_frame *const *frames, int n, float tol, int max_it,
                              int *iters, float *rel_res, float *elapsed_ms);
/* Diagnostic of the solver behind vm_poisson_extend* / vm_frame_quadratic_path (the reference: MKL DSS, Algorithm/PoissonExt.cpp:321-329,
 * timed by clock() around CPoissonExt::run, :21, 38-39): on != 0 arms a probe that brackets every launch of the solver's
 * dominant kernel -- the one that carries the PCG update x += alpha p, r -= alpha q, r.r: the level-0 restriction of the multigrid
 * cycle with the update fused in (76 bytes per unknown), or k_mgb_update by itself (a pure stream of 73 bytes per unknown) where a
 * system is too small to have a level-0 restriction -- with HIP events on the context's stream; on == 0 disarms it and returns the summed
 * event time (microseconds), the number of launches, the number of active systems summed over them and how many of the launches
 * were of the fused form.  Any of the four may be NULL.  bench.py's `poisson_extend_1080p_ex192.roofline.dominant_kernel`. */
int  vm_dbg_poisson_profile(vm_ctx *ctx, int on, double *update_us, int *update_launches, double *active_systems, int *fused_launches);
/* Read-only views of that solver's preconditioner, for tests that pin it stage by stage (the reference has no counterpart: MKL DSS
 * factorises the matrix CPoissonExt::poissonExtend assembles, Algorithm/PoissonExt.cpp:214-329; CQuadraticPath::optimize runs plain
 * CG, Algorithm/QuadraticPath.cpp:173-215).  `which`: side 1 or 2 of the frame's Poisson extension, or VM_DBG_MGB_QPATH, the
 * quadratic path's whole-grid system.  They run the solver's own set-up and cycle on the solver's own workspace, from the canvas
 * as it stands (classified, not filled: the canvases, v and u are not touched), one system, in the context's reduction mode.
 * vm_dbg_mgb_setup builds the hierarchy and reports its number of levels, the first level of the one-workgroup tail, and per level
 * (arrays of 14 entries at most) the grid's size, the smoothing sweeps each way and the numbers of 64x4-cell blocks and 64x16-cell
 * tiles that hold an unknown.  Any output may be NULL. */
#define VM_DBG_MGB_QPATH 3
int  vm_dbg_mgb_setup(vm_frame *f, int which, int *nlev, int *tail, int *w, int *h, int *nu, int *nblocks, int *ntiles);
/* Level l of the hierarchy the last vm_dbg_mgb_setup / _cycle of this system left in the frame (VM_E_STATE if there is none; launches
 * nothing): the diagonal and the weights of the edges to the east / south neighbour, h x w floats each (level 0: decoded from its
 * one byte per cell), and the level's right-hand side b and result x of the last cycle, h x w x 3 floats, where they stand in
 * memory: down to the first level of the tail.  *have: bit 0 = b, bit 1 = x were delivered.  Cells without an unknown (dg == 0)
 * of b and x hold whatever the memory held.  Any output may be NULL. */
int  vm_dbg_mgb_level(vm_frame *f, int which, int l, float *dg, float *we, float *ws, float *b, float *x, int *have);
/* One cycle z = M^-1 r of that hierarchy (rebuilt) as iteration 0 of the PCG runs it: r_in (h x w x 3 floats, zero off the
 * unknowns) is the residual; z_out = z, q_out = A z, zero off the unknowns.  z_out / q_out may be NULL. */
int  vm_dbg_mgb_cycle(vm_frame *f, int which, const float *r_in, float *z_out, float *q_out);
/* CQuadraticPath::optimize for one frame, Algorithm/QuadraticPath.cpp:24-223
 * (QuadraticPath.h:14-24): from the frame's halfway field v the per-pixel optimal
 * Jacobian blend and the Neumann Poisson solve for the quadratic motion path u,
 * which stays in the frame where vm_render_halfway reads it (the reference's
 * `_qpath`).  Multigrid-preconditioned CG to the relative residual `tol` instead
 * of 10 001 plain CG iterations; the zero-mean solution.  float32 attains about
 * 1e-4 .. 1e-5 here (|u| >> |right-hand side|; a solved, rounding-rough field: 1e-4): the best iterate
 * is delivered, VM_E_NUMERIC if its residual exceeds `tol` -- or if v folds over so that
 * the two Jacobians' columns are anti-parallel somewhere (0/0 in QuadraticPath.cpp:96-101:
 * the reference propagates the NaN).  iters/rel_res may be NULL. */
int  vm_frame_quadratic_path(vm_frame *f, float tol, int max_it,
                             int *iters, float *rel_res, float *elapsed_ms);
/* the frame's quadratic path (Pyramid::_qpath, Pyramid.h:42), tight (h, w, 2) floats */
int  vm_frame_download_qpath(vm_frame *f, float *u_xy);
/* the frame's v (set by vm_frame_upload / _set_v_from_level / _set_v_from_video), tight (h, w, 2) floats */
int  vm_frame_download_v(vm_frame *f, float *v_xy);

/* ---- synchronisation stage ("(later)" row) ------------------ */
/* Before the morph the reference's app aligns the two videos in time: the user
 * ties points of video 0 to points of video 1 -- possibly on DIFFERENT frames --
 * and CSyncThread (Algorithm/SyncThread.h:7-39, SyncThread.cpp) solves for a smooth
 * field (x, y, frame displacement) per voxel of a decimated (x, y, t) pyramid:
 * per level three conjugate-gradient solves of one thin-plate + constraint system
 * (optimize_level, SyncThread.cpp:290-480), level to level by Kernel_upsample
 * (upsample.cu:343-375).  render_resample_image (render.cu:99-246) then re-times
 * both videos with the field and the forward optical flows.  vm_sync is
 * CSyncThread's state plus the four layered arrays Pyramid::build(video0, video1,
 * f0, f1, start_res) keeps for that renderer (pyramid.cu:57-141). */
typedef struct vm_sync vm_sync;
/* a Connect between Conp lp[li] and rp[ri] (parameters.h:16-26): full-resolution
 * pixel and frame on either side, integers as in the reference */
typedef struct {
    int lx, ly, lz, rx, ry, rz;
} vm_sync_constraint;
typedef struct {
    int    iters;          /* passes of the CG loop: floor(max_iter) + 1 (`k <= _max_iter`)  */
    int    launches;
    double voxel_iters;    /* iters * W * H * D  (_current_iter += N, SyncThread.cpp:463)   */
    float  elapsed_ms;     /* HIP-event time of the level                                   */
    float  resid[3];       /* r . r of the x, y, z systems when the loop ended              */
} vm_sync_progress;
/* level geometry of Pyramid::build(video0, video1, f0, f1, start_res), pyramid.cu:143-163:
 * entry 0 is the full-resolution placeholder, entries 1.. are solved (finest first);
 * writes at most `cap` entries, *n_out = the number of levels */
int  vm_sync_level_table(int w, int h, int d, int start_res, int *lw, int *lh, int *ld, int cap, int *n_out);
/* nlevels entries (placeholder included), uses the context's w_ui / w_tps (vm_set_params) */
int  vm_sync_create(vm_ctx *ctx, int nlevels, const int *w, const int *h, const int *d, vm_sync **out);
void vm_sync_destroy(vm_sync *s);
int  vm_sync_set_constraints(vm_sync *s, const vm_sync_constraint *c, int n);
/* CSyncThread::load_identity / upsample_level (SyncThread.cpp:86-128): allocate level lvl's
 * field, zero or upsampled from lvl + 1 (which is released, as there) */
int  vm_sync_load_identity(vm_sync *s, int lvl);
int  vm_sync_upsample_level(vm_sync *s, int lvl);
/* CSyncThread::optimize_level(el): the loop runs while k <= max_iter and *run_flag (polled every
 * 64 iterations; NULL = never cancelled) */
int  vm_sync_optimize_level(vm_sync *s, int lvl, float max_iter, volatile const int *run_flag,
                            vm_sync_progress *out);
/* CSyncThread::run (SyncThread.cpp:58-84): all levels, coarsest first, max_iter * 10 halved per
 * level; out (optional) has nlevels - 1 entries, [lvl - 1] for level lvl */
int  vm_sync_solve(vm_sync *s, float max_iter, volatile const int *run_flag, vm_sync_progress *out);
/* d_x[lvl], d_y[lvl], d_z[lvl]: tight (d, h, w) float arrays (any may be NULL) */
int  vm_sync_get_field(vm_sync *s, int lvl, float *x, float *y, float *z);
int  vm_sync_set_field(vm_sync *s, int lvl, const float *x, const float *y, const float *z);
/* CSyncThread::update_result (SyncThread.cpp:482-521) for one frame: Pyramid::_vector[frame],
 * (h0, w0) float4 = (X ratio_x, Y ratio_y, Z, 0) resized to full resolution; vec4 may be NULL
 * (the frame's field is then only refreshed on the device, where vm_sync_render reads it) */
int  vm_sync_result(vm_sync *s, int lvl, int frame, float *vec4);
/* the layered arrays of Pyramid::build (pyramid.cu:93-141): frame `frame` of video `side`
 * (RGBA8, alpha ignored) and of its forward flow (float2) */
int  vm_sync_upload_frame(vm_sync *s, int side, int frame, const uint8_t *rgba, int pitch_bytes);
int  vm_sync_upload_flow(vm_sync *s, int side, int frame, const float *flow_xy, int pitch_floats);
/* render_resample_image(out, ..., fa, frame, ...) (render.cu:203-246; caller RenderWidget::
 * RenderStage1, UI/RenderWidget.cpp:205-227) with this frame's field as it stands: the result of
 * the level vm_sync_result last delivered from, if that level still holds a field, else of level 1
 * if it holds one, else zero.  Only one frame's result is kept on the device, and every call that
 * changes a field (load_identity, upsample_level, optimize_level, solve, set_field) drops it, so
 * the render regenerates it whenever the frame or a field changed; rgb_out: h0 rows of
 * pitch_bytes, RGB8 */
int  vm_sync_render(vm_sync *s, float fa, int frame, uint8_t *rgb_out, int pitch_bytes);
/* the same, result left on the device (timing without the download) */
int  vm_sync_render_dev(vm_sync *s, float fa, int frame, float *elapsed_ms);

/* ---- dense optical flow ---------------------------------------------------- */
/* MdiEditor::OpticalFlow, UI/MdiEditor.cpp:1584-1689: the reference converts each frame to grey and
 * runs cuda::FarnebackOpticalFlow with its defaults.  Here: Farneback's two-frame polynomial-expansion
 * method written from the published method, on the device (DESIGN.md 3.6 states the spec; it is not
 * bit-compatible with OpenCV).  A flow d maps frame a to frame b: b(x + d(x)) ~ a(x).  Supported:
 * num_levels >= 0, 0 < pyr_scale < 1, odd win_size in 3..31, num_iters >= 1, poly_n 5 or 7,
 * poly_sigma > 0; fast_pyramids and flags must be 0; frames at least 32 x 32.  Everything else is
 * VM_E_INVALID.  Results do not depend on how many flows share a call. */
typedef struct {
    int   num_levels;
    float pyr_scale;
    int   fast_pyramids;
    int   win_size;
    int   num_iters;
    int   poly_n;
    float poly_sigma;
    int   flags;
} vm_flow_params;
/* the reference's values (cuda::FarnebackOpticalFlow defaults, UI/MdiEditor.cpp:1584-1689); no device needed */
int  vm_flow_params_default(vm_flow_params *p);
/* n independent flows a[i] -> b[i] of one size (UI/MdiEditor.cpp:1584-1689), all in the same launches;
 * host frames in (RGB8 rows of pitch_bytes, or float luma rows of `pitch` floats; 0 = tight),
 * flow_xy[i] = tight (h, w, 2) floats out; p == NULL: the defaults */
int  vm_optical_flow_rgb(vm_ctx *ctx, int w, int h, int n, const uint8_t *const *a, const uint8_t *const *b,
                         int pitch_bytes, const vm_flow_params *p, float *const *flow_xy);
int  vm_optical_flow_luma(vm_ctx *ctx, int w, int h, int n, const float *const *a, const float *const *b,
                          int pitch, const vm_flow_params *p, float *const *flow_xy);
/* MdiEditor::OpticalFlow of both videos (UI/MdiEditor.cpp:1584-1689) followed by the flow half of
 * Pyramid::build (as vm_video_build_flows): rgb0[t] / rgb1[t] = the depth0 frames of video 0 / 1;
 * f[t] = frame t -> t + 1 (zero for the last frame), b[t] = t -> t - 1 (zero for frame 0).  The
 * flows never leave the device; the pages get what vm_video_build_flows would give them for the
 * flows vm_optical_flow_rgb returns. */
int  vm_video_build_flows_rgb(vm_video *v, const uint8_t *const *rgb0, const uint8_t *const *rgb1,
                              int pitch_bytes, const vm_flow_params *p);
/* forward flows of both videos (UI/MdiEditor.cpp:1584-1689) from the frames vm_sync_upload_frame put
 * there, into the layered flow arrays of pyramid.cu:93-141 (the last frame's flow is zero): what
 * vm_sync_upload_flow of the same flows would leave */
int  vm_sync_compute_flows(vm_sync *s, const vm_flow_params *p);

/* ---- key-point tracks of stage 2 ------------------------------------------- */
/* MdiEditor keeps the full-resolution frames and flows of both videos (resample1/2, f1/f2, b1/b2) and
 * walks every user key-point through the other frames of its video along them: AddPoint
 * (UI/MdiEditor.cpp:1230-1276), MovePoint (:1279-1393), each propagated point weighed by the histogram
 * correlation of its patch against the key's (Histo, :1516-1582).  vm_track holds that data on the
 * device; vm_track_propagate computes any number of track segments in one launch.  The arithmetic is
 * stated in DESIGN.md 3.7 (tests/track_ref.py); side 0 = the left video, 1 = the right. */
typedef struct vm_track vm_track;
/* a track segment.  Chain (ofr < 0): from key (x, y, frame) in direction dir (+1 / -1) up to the last /
 * first frame, AddPoint's loops and MovePoint's with no key on that side.  Blend (ofr >= 0): the frames
 * strictly between the moved key (x, y, frame) and the neighbouring key (ox, oy, ofr), MovePoint's
 * blend of the two chains (:1315-1339, :1368-1392); dir is 0 or the sign of ofr - frame. */
typedef struct {
    int side;
    int x, y, frame;
    int ox, oy, ofr;
    int dir;
} vm_track_segment;
/* a propagated point (Conp with w = 0): position and weight */
typedef struct {
    int   x, y;
    float weight;
} vm_track_point;
/* frames w x h (at least 32 x 32, as the flow), `depth` frames per video (1..16384) */
int  vm_track_create(vm_ctx *ctx, int w, int h, int depth, vm_track **out);
void vm_track_destroy(vm_track *t);
/* one RGB8 frame of video `side` (pitch_bytes; 0 = tight) */
int  vm_track_upload_frame(vm_track *t, int side, int frame, const uint8_t *rgb, int pitch_bytes);
/* f[frame] (frame -> frame + 1) and b[frame] (frame -> frame - 1) of video `side`, tight rows of
 * `pitch` floats (0 = 2 w); either may be NULL (left as it is).  Every value must be finite and within
 * +-1e5 px (VM_E_INVALID otherwise): with keys within +-1e6 px every position stays an int. */
int  vm_track_upload_flows(vm_track *t, int side, int frame, const float *f_xy, const float *b_xy, int pitch);
/* MdiEditor::OpticalFlow (:1584-1689) of both uploaded videos, as vm_video_build_flows_rgb computes
 * them; f[depth - 1] and b[0] are zero */
int  vm_track_compute_flows(vm_track *t, const vm_flow_params *p);
/* the flows of (side, frame) back to the host; either output may be NULL */
int  vm_track_get_flows(vm_track *t, int side, int frame, float *f_xy, float *b_xy);
/* n segments in one launch: segment i writes out[i * depth + s] for every frame s it covers and
 * nothing else.  VM_E_INVALID for a bad side / frame / direction, equal key frames of a blend or a key
 * beyond +-1e6 px,
 * VM_E_STATE when a frame or flow the segment reads was never supplied. */
int  vm_track_propagate(vm_track *t, const vm_track_segment *seg, int n, vm_track_point *out);
/* the flow half of Pyramid::build (as vm_video_build_flows) from the tracker's flows: NextStage's one
 * OpticalFlow (:1714-1791) serves the tracks and the stage-2 pyramid.  The sizes must match. */
int  vm_video_build_flows_track(vm_video *v, const vm_track *t);

/* ---- multi-GPU ----------------------------------------------------------- */
/* The shared parameter block every rank needs (KernParameters + iteration
 * control + constraints), flattened so that any transport -- the RCCL
 * broadcast of bench.py / the C++ driver -- can ship it. */
typedef struct {
    vm_kern_params kp;
    float max_iter, max_iter_drop_factor;
    int   start_res, math_mode, n_constraints;
} vm_param_block;
/* in-place RCCL broadcast of `bytes` at device pointer `dev_buf` from rank
 * `root` on communicator `nccl_comm` (an ncclComm_t), on the context's stream */
int  vm_rccl_bcast(vm_ctx *ctx, void *nccl_comm, void *dev_buf, uint64_t bytes, int root);
/* One PROCESS driving n devices (SURVEY 7 step 9, 8(b) `vm_bcast_params`; the reference is single-GPU,
 * UI/MdiEditor.cpp:54-75 picks one device): ncclCommInitAll over `devices` (n distinct ordinals) -> comms_out[n];
 * vm_rccl_comm_destroy frees one. */
int  vm_rccl_comm_init_all(int n, const int *devices, void **comms_out);
void vm_rccl_comm_destroy(void *nccl_comm);
/* The shared parameter block from ctxs[root] to all n contexts over RCCL (one ncclBroadcast per communicator
 * inside one ncclGroup, each on its context's stream); every context then sets its kernel parameters and
 * arithmetic mode from the copy IT received.  blocks_out: n entries (may be NULL), the block as received.
 * comms == NULL is a TEST MODE for contexts sharing one device (RCCL wants one rank per device): the copies go
 * device-to-device on that device instead. */
int  vm_bcast_params(vm_ctx *const *ctxs, void *const *nccl_comms, int n, int root,
                     const vm_param_block *blk, vm_param_block *blocks_out);
/* The same one broadcast for a payload of the caller's length -- BASELINE config[4]: the parameter block followed by the
 * frames' point constraints (Parameters::lp / rp / cnt resolved to vm_constraint rows, parameters.h:16-26, consumed at
 * Algorithm/morph.cu:345-388, 471-505), the layout videomorphing_amd/dist.py:pack_block ships between processes.  `src`
 * (host, `bytes` long) goes from ctxs[root] to all n contexts over RCCL (nccl_comms == NULL: the one-device test mode
 * of vm_bcast_params); dst_host[i] (host, `bytes` each) receives what context i got.  Nothing is interpreted. */
int  vm_bcast_bytes(vm_ctx *const *ctxs, void *const *nccl_comms, int n, int root, const void *src, uint64_t bytes,
                    void *const *dst_host);

#ifdef __cplusplus
}
#endif
#endif
