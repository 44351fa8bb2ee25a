// vm_host.h -- host-side objects behind the opaque handles of include/vmorph.h.
#ifndef VM_HOST_H
#define VM_HOST_H

#include "vm_internal.h"
#include "vm_devmem.h"
#include <mutex>
#include <vector>

struct vm_ctx;
bool vm_ctx_alive(const vm_ctx *c); // vm_api.cpp: is this context still alive?

#define VM_HIP(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            return vm_fail(VM_E_DEVICE, "%s:%d %s: %s", __FILE__, __LINE__, #call,         \
                           hipGetErrorString(e_));                                         \
    } while (0)

// HIP's current device belongs to the calling host thread, and the API is driven from worker
// threads (MatchingThread, thread pools): every entry point that allocates or launches makes
// the context's device current first and restores the caller's device on return.
struct VmDeviceGuard {
    int prev = -1;
    bool switched = false;
    bool ok = true; // false: the device could not be made current -- nothing may be launched
    explicit VmDeviceGuard(int dev)
    {
        // HIP's "last error" is per thread and sticky across libraries: an error another
        // library left behind (RCCL probing peers, a framework's failed query) must not be
        // reported by the hipGetLastError() checks that follow this entry point's launches
        (void)hipGetLastError();
        if (hipGetDevice(&prev) != hipSuccess || prev != dev) {
            ok = hipSetDevice(dev) == hipSuccess;
            switched = ok && prev >= 0;
            (void)hipGetLastError();
        }
    }
    ~VmDeviceGuard()
    {
        if (switched)
            (void)hipSetDevice(prev);
    }
    VmDeviceGuard(const VmDeviceGuard &) = delete;
    VmDeviceGuard &operator=(const VmDeviceGuard &) = delete;
};
#define VM_CAT2(a, b) a##b
#define VM_CAT(a, b) VM_CAT2(a, b)
// In functions that return a status: a device that cannot be made current is an error, not a
// launch on whatever device the calling thread happened to have.
#define VM_ON_DEVICE(ctx)                                                                          \
    VmDeviceGuard VM_CAT(vm_device_guard_, __LINE__)((ctx)->device);                                \
    if (!VM_CAT(vm_device_guard_, __LINE__).ok)                                                    \
        return vm_fail(VM_E_DEVICE, "%s: device %d cannot be made current", __func__, (ctx)->device)
// ... and in destructors / void functions (best effort)
#define VM_ON_DEVICE_VOID(ctx) VmDeviceGuard VM_CAT(vm_device_guard_, __LINE__)((ctx)->device)

// The guard of the C-ABI's entry points, for a handle with a `ctx` member or a bare vm_ctx *: not NULL -> its context
// alive (nothing of a destroyed one is read) -> VM_ENTER_LOCKED only: ctx->mu held to the end of the function -> the
// device current.  Which form an entry point uses belongs to the locking contract (vm_frame_set_v_from_level).
inline vm_ctx *vm_ctx_of(vm_ctx *c) { return c; }
template <class T> vm_ctx *vm_ctx_of(T *o) { return o->ctx; }
#define VM_GUARD(obj, locked)                                                                                         \
    if (!(obj)) return vm_fail(VM_E_INVALID, "%s: NULL handle", __func__);                                            \
    vm_ctx *const VM_CAT(vm_guard_ctx_, __LINE__) = vm_ctx_of(obj);                                                   \
    if (!vm_ctx_alive(VM_CAT(vm_guard_ctx_, __LINE__)))                                                               \
        return vm_fail(VM_E_INVALID, "%s: the context was destroyed", __func__);                                      \
    std::unique_lock<std::recursive_mutex> VM_CAT(vm_guard_lock_, __LINE__)(VM_CAT(vm_guard_ctx_, __LINE__)->mu, std::defer_lock); \
    if (locked) VM_CAT(vm_guard_lock_, __LINE__).lock();                                                              \
    VM_ON_DEVICE(VM_CAT(vm_guard_ctx_, __LINE__))
#define VM_ENTER(obj) VM_GUARD(obj, false)
#define VM_ENTER_LOCKED(obj) VM_GUARD(obj, true)

struct VmMgbSys; // vm_mgb.h

struct vm_ctx {
    std::recursive_mutex mu;         // a context is single-threaded by contract; this makes misuse safe
    int device = 0;
    int math_mode = VM_MATH_EXACT;
    vm_kern_params kp{};
    // a plain handle, destroyed by ctx_free after every member (vm_api.cpp): ensure_lanes (vm_video.cpp) replaces a
    // lane's stream
    hipStream_t stream = nullptr;
    VmEvent ev0, ev1;
    // done_ev: recorded on `stream` (under `mu`, never inside a graph capture) whenever a solver call has enqueued its
    // last write of a level; xfer_ev: scratch for the same purpose in a consumer that holds `mu` itself.  Another
    // context's stream waits on one of them instead of the host draining this stream (vm_frame_set_v_from_level)
    VmEvent done_ev, xfer_ev;
    VmDev<uint32_t> tables;          // VM_TAB_WORDS words
    VmDev<uint32_t> flags;           // per-iteration "improving" flags
    VmPinned<uint32_t> flags_host;   // ... mirror
    VmDev<uint32_t> stats;           // per-iteration activity counters, VM_STAT_WORDS words each
    VmPinned<uint32_t> stats_host;   // ... mirror
    VmDev<uint32_t> step_slots;      // STEP schedule: per-workgroup activity counts of the last two launches (two halves)
    // PASS schedule: tile-barrier counters (one per tile group and launch of a batch), the
    // error word a timed-out barrier raises (+ pinned mirror), optional XCD-placement record
    VmDev<uint32_t> pass_bar;
    VmDev<uint32_t> pass_err;
    VmPinned<uint32_t> pass_err_host;
    int pass_resident[16] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}; // co-resident k_pass workgroups on this device, per arithmetic build and sweep variant (math_mode * 2 + temporal); -1: not asked yet
    VmDev<uint32_t> pass_dbg;        // vm_dbg_pass_xcd: 256 words, XCC id per workgroup of the last launch
    VmDev<char> pass_snap;           // AUTO: the levels' slabs as they stood before the current PASS batch
    bool pass_latched_off = false;   // AUTO: a tile barrier timed out once on this context: STEP from then on
    bool pass_latched_by_test = false; // ... and it was vm_dbg_pass_force_timeout's doing (only then the hook may lift it)
    int pass_fallbacks = 0;          // how often that happened (vm_dbg_pass_fallbacks)
    int pass_test_timeout = 0;       // vm_dbg_pass_force_timeout: the next PASS launches behave as if a barrier timed out
    int sweep_threads = 0;           // 0 = automatic
    int sweep_mode = 0;              // VM_SWEEP_AUTO / TILE / SPLIT
    int sweep_parts = 0;             // workgroups per tile in the SPLIT schedule, 0 = automatic
    VmDev<VmLevelView> views;        // device copies of the level views of the current batch
    VmDev<vm_constraint> cons_dev;
    // hipGraph replay of launch-bound TILE sweeps (vm_sweep_sched.cpp): 8 iterations per graph
    VmDev<int> iter_dev;             // device iteration counter read by the replayed kernels
    struct SweepGraph {
        int math_mode;
        int n, w, h, cap, fixed_work, threads, dense, order;
        int temporal; // the sweep variant its kernel nodes were captured with (SweepRun::temporal)
        const void *views, *flags, *stats, *tile_list;
        vm_kern_params kp;
        hipGraphExec_t exec;
    };
    std::vector<SweepGraph> graphs;
    int commit_order = 0;         // vm_set_commit_order (EXACT, diagnostic): order 0..3
    int sweep_variant = 0;        // vm_dbg_sweep_variant: 0 = by the level (the kernels without the temporal term where no page carries it), 1 = always the general kernels
    int sparse_resident = 0;      // vm_dbg_sparse_resident: 0 = automatic, 1 = never, 2 / 3 = tests (k_sparse, sv_phases)
    unsigned long long sparse_resident_visits = 0; // vm_dbg_sparse_resident_visits: tile visits served from the resident LDS copy
    VmDev<uint32_t> tile_list;       // the listed form of pruned TILE passes over big batches (k_tile_scan): counters, stamps, entries
    int use_graphs = -1;             // -1: not decided yet, 0: off (VM_NO_GRAPH or a failed capture), 1: on
    VmDev<VmMgbSys> mgb_sys;         // device descriptors of the systems of the current Poisson batch (vm_poisson_api.cpp)
    VmDev<char> mgb_shared;          // ... and their PCG scalars + block / tile counts, contiguous: ONE clear and ONE read-back per check for the whole batch
    // vm_dbg_poisson_profile: HIP-event time of the launch that carries the PCG update (k_mgb_update, or the level-0
    // restriction with the update fused in), summed over the launches of the solves since the probe was switched on,
    // and what those launches processed
    // vm_set_reduction: VM_REDUCE_ATOMIC (0) or VM_REDUCE_ORDERED (1), how the batched PCG and the quadratic path's mean
    // shift reduce (vm_mgb.h); mgb_ord: the ordered mode's partials, tickets and group sums of the current batch
    int reduction = 0;
    VmDev<char> mgb_ord;
    // the error view (vm_error.cpp): jobs, workgroup partials and totals of the current call; arrival counters (zero between
    // calls); the plane or image on its way to the host; pinned staging of the jobs (in) and the totals (out)
    VmDev<char> err_ws;
    VmDev<unsigned> err_tickets;
    VmDev<char> err_out;
    VmPinned<char> err_host;
    bool mgb_prof = false;
    double mgb_prof_us = 0, mgb_prof_unknown_launches = 0;
    int mgb_prof_launches = 0, mgb_prof_fused = 0;
};

// A launch on the context's stream, timed by HIP events if `ms` is given: ev0, fn() (which enqueues), the launch error,
// then ev1 recorded and waited for and the elapsed time read.  Without `ms` nothing is waited for.
template <class F> int vm_timed_launch(vm_ctx *c, float *ms, F fn)
{
    if (ms) VM_HIP(hipEventRecord(c->ev0.get(), c->stream));
    fn();
    VM_HIP(hipGetLastError());
    if (ms) {
        VM_HIP(hipEventRecord(c->ev1.get(), c->stream));
        VM_HIP(hipEventSynchronize(c->ev1.get()));
        VM_HIP(hipEventElapsedTime(ms, c->ev0.get(), c->ev1.get()));
    }
    return VM_OK;
}

struct vm_level {
    int w = 0, h = 0, rs = 0, imp_rs = 0, imp_rows = 0;
    VmDev<char> slab;
    VmDev<char> ws;                  // SPLIT / STEP workspace, allocated on first use (vm_sweep_sched.cpp)
    VmDev<char> sp_ws;               // SPARSE workspace (word lists, stamps), allocated on first use
    bool has_state = false;
    VmLevelView view{};
    // pages of a video level: where lvl.temp.ref / lvl.temp.mask of the page live (the view
    // points at them only while the page is swept with flag == true)
    float2 *temp_ref_store = nullptr;
    float *temp_mask_store = nullptr;
};

struct vm_pyr {
    vm_ctx *ctx = nullptr;
    int device = 0;                  // of ctx: the buffers can be freed after the context is gone
    std::vector<vm_level> lv;
};

// One page of a video level: the level state of one frame pair plus what couples it to its
// neighbours in time -- the four flow fields of the page (PyramidLevel::f0/f1/b0/b1,
// Pyramid.h:85-90, pitched float2 instead of cudaArray) and lvl.temp.ref / lvl.temp.mask.
struct vm_video_page {
    vm_level lv;
    VmDev<char> tslab;                                       // flows + temporal arrays
    float2 *flow[4] = {nullptr, nullptr, nullptr, nullptr};  // f0, f1, b0, b1
    float2 *temp_ref = nullptr;
    float *temp_mask = nullptr;
};

// The stage-2 pyramid of a video pair (class Pyramid with depth > 1, Pyramid.h:14-48):
// level l holds depth[l] pages; level 0 finest, the last level holds only v.
// A lane of the level pipeline of vm_video_solve: its own stream and sweep scratch (a context of
// its own on the same device) and its own splat accumulators, so that independent (level, chain
// step) tasks can run side by side (vm_video.cpp).
struct vm_video_lane {
    vm_ctx *c = nullptr;
    VmDev<long long> acc;
};

struct vm_video {
    vm_ctx *ctx = nullptr;
    int device = 0;
    int depth0 = 1;                       // frames of the video (the placeholder level's depth)
    std::vector<int> depth;               // pages per level
    std::vector<int> factor_t;            // temporal stride the level was built with (pyramid.cu:468)
    std::vector<float> factor_d;          // per level (pyramid.cu:470-477); factor_d0 for the placeholder
    float factor_d0 = 1.0f;
    std::vector<std::vector<vm_video_page>> pages;
    // scratch of the splat (sized for the largest level with temporal state): fixed-point accumulators, v_cur, weight
    VmDev<long long> acc;
    VmDev<float2> vcur;
    VmDev<float> weight;
    std::vector<vm_video_lane> lanes;     // created by the first pipelined solve
    VmDev<float2> result_tmp;             // vm_frame_set_v_from_video: two full-resolution planes (blended frames)
};

struct vm_frame {
    vm_ctx *ctx = nullptr;
    int device = 0;
    int w = 0, h = 0, ex = 0, cw = 0, ch = 0, rs = 0;
    VmDev<uchar4> ext[2];                 // (w+2ex) x (h+2ex) RGBA8 canvases
    VmDev<uchar4> crop[2];                // w x h originals (CPoissonExt::_image1/_image2, PoissonExt.cpp:26-27)
    VmDev<float2> v, u;                   // h x rs
    bool u_zero = true;                   // the quadratic path is all zeros (never uploaded / computed: the reference app's
                                          // state, UI/MdiEditor.cpp:1898-1903): vm_render_halfway then skips its 21 taps of u --
                                          // a zero path stays zero through the fixed-point steps, the bytes are the same
    VmDev<uint8_t> out;                   // h x w x 3
    VmDev<uint8_t> rgb_stage;             // vm_frame_upload_rgb: the two RGB8 frames as they arrive (2 x h x w x 3), allocated on first use
    // solver workspace (allocated on first use), pws2[side - 1]: one per side (both sides of a frame are in flight
    // together); the quadratic path uses side 1's
    VmDev<char> pws2[2];
    // float layers carried through the morph (vm_frame_upload_layers, vm_warp.cpp), allocated on the first upload: two tight
    // (h, w, layer_ch) images, the second at layer_off floats; layer_ch == 0: the frame holds none
    VmDev<float> layers;
    int layer_ch = 0;
    size_t layer_off = 0;
    // ... and their Poisson extension (vm_frame_extend_layers, vm_poisson_api.cpp), allocated on the first call: two
    // (ch, cw, layer_ch) canvases with the image at (ex, ex), the second at lext_off floats; the byte planes that tell
    // where a canvas cell holds a value (two of cw x ch); one word per system and channel group, raised by a right-hand
    // side that is not all zeros.  layer_ext: the render calls sample the canvases instead of the tight layers; a new
    // upload of layers drops it
    VmDev<float> lext;
    VmDev<uint8_t> lext_valid;
    VmDev<int> lext_nz;
    size_t lext_off = 0;
    bool layer_ext = false;
    // what the warp kernels write before it goes to the host (the maps of vm_warp.cpp, the output of a render call of
    // vm_render_calls.cpp), allocated on first use
    VmDev<char> warp_out;
    // the transition schedule (vm_frame_upload_schedule, vm_warp.cpp), allocated on the first upload: the geometry plane and
    // the colour plane of h x rs pairs (t0, t1), then the scratch plane of the same size a call ramps its rates into
    VmDev<float2> sched;
    bool has_sched = false;
    // the start points of a carry call (vm_frame_carry_points, vm_render_calls.cpp), grown on demand
    VmDev<float2> carry_pts;
    // the pyramids of a multiband call (vm_frame_render_multiband, vm_render_calls.cpp; the layout is vm_multiband.h's),
    // allocated on first use and grown when the channels or the levels ask for more; mb_levels == 0: no call yet.
    // mb_channels / mb_layers: what the last call blended (vm_dbg_multiband_level)
    VmDev<float> mb;
    int mb_levels = 0, mb_channels = 0;
    bool mb_layers = false;
};

// The one destroy path of the objects that live on a context's device (pyramid, video, frame, sync).  With the device
// current and whatever may still use the object's buffers drained -- the context's stream, or the whole device once the
// context is gone (a garbage-collected host language can destroy in that order; the object remembers its device) -- the
// object is deleted and its members free themselves.  If the device cannot be made current, the object and its buffers
// are leaked on purpose rather than freed on another device.
template <class T> void vm_destroy_object(T *o)
{
    if (!o) return;
    VmDeviceGuard g(o->device);
    if (!g.ok) return;
    if (vm_ctx_alive(o->ctx)) {
        std::lock_guard<std::recursive_mutex> lock(o->ctx->mu);
        (void)hipStreamSynchronize(o->ctx->stream);
        delete o;
    } else {
        (void)hipDeviceSynchronize();
        delete o;
    }
    (void)hipGetLastError();
}

// level-wise pieces of the solver shared by the frame-pair API (vm_api.cpp) and the video
// API (vm_video.cpp); a "level" here is one page of one pyramid level
int vm_level_alloc(vm_ctx *c, vm_level &l, bool with_images);
int vm_level_upsample(vm_ctx *c, vm_level &dst, const vm_level &src);
int vm_level_init(vm_ctx *c, vm_level &l, int w0, int h0, const vm_constraint *cons, int n);
int vm_level_read_field(vm_ctx *c, vm_level &l, int field, void *host);
// ... and its copies from / to the host (drained on return): pitch in floats, 0 = tight; fn names the entry point;
// `kind` = hipMemcpyHostToDevice writes v, hipMemcpyDeviceToHost reads it into v
int vm_level_write_luma(vm_ctx *c, vm_level &l, const float *img0, const float *img1, int pitch, const char *fn);
int vm_level_copy_v(vm_ctx *c, vm_level &l, hipMemcpyKind kind, const float *v, int pitch, const char *fn);
// A caller's host image of h rows: `pitch` counts units of `unit` bytes (what include/vmorph.h documents for the entry
// point fn: floats 4, bytes 1), 0 = tight.  vm_pitch_resolve turns 0 into the row and refuses a pitch below it;
// vm_copy_pitched does that and copies the rows to or from a device image of dev_pitch_bytes (by `kind`) on s.
int vm_pitch_resolve(const char *fn, int *pitch, size_t unit, size_t row_bytes);
int vm_copy_pitched(const char *fn, hipMemcpyKind kind, void *dev, size_t dev_pitch_bytes, const void *host, int pitch,
                    size_t unit, size_t row_bytes, int h, hipStream_t s);
// The three planes of a frame's schedule (vm_warp.cpp, which uploads them; the maps call there and the render calls of
// vm_render_calls.cpp bind them): geometry, colour, and the scratch plane a call ramps its rates into.
void vm_frame_schedule_planes(vm_frame *f, const float2 **geo, const float2 **color, float2 **rates);
// the sweep of one level (vm_sweep_sched.cpp)
int vm_iteration_cap(float max_iter, int *cap);
int vm_optimize_levels(vm_ctx *c, vm_level **lv, int n, float max_iter, volatile const int *run_flag,
                       int fixed_work, vm_progress *out);

// Morph::cpu_optimize_level (morph.cu:419-590) on the host: v_out is a tight
// (h, w, 2) array
int vm_host_coarse_solve(int w, int h, int w0, int h0, const vm_kern_params &kp,
                         const vm_constraint *cons, int n, float *v_out, int depth = 1);

#endif
