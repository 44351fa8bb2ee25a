// vm_sweep_sched.cpp -- the host driver of the optimizer sweep: vm_optimize_levels relaxes one level of a batch of
// frame pairs (or video pages) in batches of iterations, each under the schedule vm_sweep_plan.h picks for it.
// Here: the launcher tables, the hipGraph of TILE iterations, the schedules' workspaces, the PASS token and the
// time-out recovery, and the fold of the read-back counters into vm_progress.  Kernels: vm_sweep_kernels.hip.
#include "vm_internal.h"
#include "vm_host.h"
#include "vm_sweep_plan.h"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#define VM_MAX_DEVICES_TRACKED 64

// The workspace of the SPLIT / STEP schedules (two record sets, the second copy of the sums
// and of the mask: 104 B per pixel against 72 B of solver state) is allocated the first time
// a level is swept with one of them -- in practice the small levels only.
static int level_ensure_ws(vm_ctx *c, vm_level &l)
{
    if (l.ws.get()) return VM_OK;
    const size_t n = (size_t)l.rs * l.h, nimp = (size_t)l.imp_rs * l.imp_rows;
    const size_t total = 2 * vm_align256(n * 4) + 4 * vm_align256(n * 16) + 3 * vm_align256(n * 8) + 2 * vm_align256(n * 4) + vm_align256(nimp * 4);
    if (int rc = l.ws.reserve(total)) return rc;
    char *b = l.ws.get();
    VmLevelView &V = l.view;
    V.rec_tag = (uint32_t *)b; b += vm_align256(n * 4);
    V.rec_tag2 = (uint32_t *)b; b += vm_align256(n * 4);
    V.rec_a = (float4 *)b; b += vm_align256(n * 16);
    V.rec_b = (float4 *)b; b += vm_align256(n * 16);
    V.rec_a2 = (float4 *)b; b += vm_align256(n * 16);
    V.rec_b2 = (float4 *)b; b += vm_align256(n * 16);
    V.mean2 = (float2 *)b; b += vm_align256(n * 8);
    V.var2 = (float2 *)b; b += vm_align256(n * 8);
    V.tps_b2 = (float2 *)b; b += vm_align256(n * 8);
    V.cross2 = (float *)b; b += vm_align256(n * 4);
    V.value2 = (float *)b; b += vm_align256(n * 4);
    V.impmask2 = (uint32_t *)b;
    VM_HIP(hipMemsetAsync(l.ws.get(), 0, total, c->stream));
    return VM_OK;
}

// The workspace of the SPARSE schedule (vm_sweep_kernels.hip): two lists of mask-word indices,
// their lengths and a stamp per word -- 12 B per 5x5 block, allocated on first use.
static int level_ensure_sparse(vm_ctx *c, vm_level &l)
{
    if (l.sp_ws.get()) return VM_OK;
    const size_t nw = (size_t)l.imp_rs * l.imp_rows;
    const size_t total = vm_align256(2 * nw * 4) + vm_align256(nw * 4) + 256;
    if (int rc = l.sp_ws.reserve(total)) return rc;
    char *b = l.sp_ws.get();
    l.view.sp_wl = (uint32_t *)b; b += vm_align256(2 * nw * 4);
    l.view.sp_stamp = (uint32_t *)b; b += vm_align256(nw * 4);
    l.view.sp_cnt = (uint32_t *)b;
    VM_HIP(hipMemsetAsync(l.sp_ws.get(), 0, total, c->stream));
    return VM_OK;
}

// How many workgroups the dense sweeps of SMALL levels (<= 32 tiles per pass: the 256-VGPR kernel without the
// interior form, one 512-thread workgroup = 8 waves = all of a CU's registers) have in flight on a device, summed
// over the contexts of this process that are sweeping such a level right now.  A batch of 30 pairs x 8 tiles
// = 240 workgroups fills the chip one per CU; a second stream's 240 then wait for them.  As 256-thread
// workgroups (4 waves: a tile's ~127 candidates of a phase at two lanes each; a full phase in two rounds) two
// fit a CU -- 2 x 75 KB of LDS, 2 x 4 waves x 256 VGPRs -- and the two streams' tiles run side by side, each SIMD
// with two searching waves instead of one: config[2]'s 60 pairs on one GPU 968 -> 890 ms.  It only pays when the
// workgroups in flight exceed the CUs by enough (measured: 2 x 240 and 1 x 840 yes; 1 x 240, 2 x 120 no: -16 %),
// so the rule counts them.  Results do not depend on the workgroup size (the lane fan-out per candidate, which
// orders the FAST sums, is a compile-time constant of the kernel).
static std::atomic<int> g_small_dense_wgs[VM_MAX_DEVICES_TRACKED];
struct SmallDensePresence {
    int dev = -1, wgs = 0;
    void enter(int device, int n_wgs)
    {
        if (dev >= 0 || device < 0 || device >= VM_MAX_DEVICES_TRACKED) return;
        dev = device;
        wgs = n_wgs;
        g_small_dense_wgs[dev].fetch_add(wgs);
    }
    void leave()
    {
        if (dev >= 0) g_small_dense_wgs[dev].fetch_sub(wgs);
        dev = -1;
    }
    int in_flight() const { return dev < 0 ? 0 : g_small_dense_wgs[dev].load(); }
    ~SmallDensePresence() { leave(); }
};

// the sweep launchers of one arithmetic build of vm_sweep_kernels.hip
struct SweepLaunchers {
    decltype(&vm_launch_optimize_exact) optimize;
    decltype(&vm_launch_next_iter_exact) next_iter;
    decltype(&vm_launch_optimize_sparse_exact) sparse;
    decltype(&vm_launch_optimize_split_exact) split;
    decltype(&vm_launch_optimize_step_exact) step;
    decltype(&vm_launch_optimize_pass_exact) pass;
    decltype(&vm_pass_resident_blocks_exact) pass_resident;
};
#define VM_SWEEP_LAUNCHERS(SUFFIX)                                                                          \
    {vm_launch_optimize_##SUFFIX, vm_launch_next_iter_##SUFFIX, vm_launch_optimize_sparse_##SUFFIX,         \
     vm_launch_optimize_split_##SUFFIX, vm_launch_optimize_step_##SUFFIX, vm_launch_optimize_pass_##SUFFIX, \
     vm_pass_resident_blocks_##SUFFIX}
static const SweepLaunchers &sweep_launchers(int math_mode)
{
    static const SweepLaunchers exact = VM_SWEEP_LAUNCHERS(exact);
    static const SweepLaunchers fast = VM_SWEEP_LAUNCHERS(fast);
    // VM_MATH_EXACT_FMA: the EXACT source with -ffp-contract=fast (fused multiply-adds wherever the compiler
    // contracts, IEEE division and square root): what nvcc's default --fmad=true makes of the reference source
    static const SweepLaunchers exactf = VM_SWEEP_LAUNCHERS(exactf);
    // VM_MATH_REF_FASTMATH: that source as the reference's project file compiles it (--use_fast_math)
    static const SweepLaunchers reffm = VM_SWEEP_LAUNCHERS(reffm);
    // VM_MATH_REF_TEX8 / _TRUNC: that source, IEEE, with the 8-bit bilinear weights of CUDA's texture filter
    static const SweepLaunchers tex8 = VM_SWEEP_LAUNCHERS(tex8);
    static const SweepLaunchers tex8t = VM_SWEEP_LAUNCHERS(tex8t);
    switch (math_mode) {
    case VM_MATH_FAST: return fast;
    case VM_MATH_EXACT_FMA: return exactf;
    case VM_MATH_REF_FASTMATH: return reffm;
    case VM_MATH_REF_TEX8: return tex8;
    case VM_MATH_REF_TEX8_TRUNC: return tex8t;
    default: return exact;
    }
}

static const int pass_offs[4][2] = {{0, 0}, {VM_TILE_W, 0}, {0, VM_TILE_H}, {VM_TILE_W, VM_TILE_H}}; // morph.cu:1382-1385

// A hipGraph of VM_GRAPH_ITERS TILE-schedule iterations (4 pass launches each, one counter bump)
// for the given geometry, instantiated once per context and replayed: pruned sweeps last 2-3 us
// on the GPU, less than the 4-6 us the host needs per eager launch, so the sweep loop of a
// converged or nearly converged level is launch-bound without it.  The iteration number is not
// a kernel argument there but a device counter.  Returns nullptr when graphs are unavailable
// (VM_NO_GRAPH set, or capture/instantiation failed once): the caller launches eagerly.
#define VM_GRAPH_ITERS 8
static hipGraphExec_t sweep_graph(vm_ctx *c, int math_mode, int n, int w, int h, int cap, int fixed_work, int threads,
                                  int dense, uint32_t *tile_list, int temporal, const VmKParams &P)
{
    if (c->use_graphs < 0) c->use_graphs = getenv("VM_NO_GRAPH") ? 0 : 1;
    if (!c->use_graphs) return nullptr;
    for (auto &g : c->graphs)
        if (g.math_mode == math_mode && g.n == n && g.w == w && g.h == h && g.cap == cap && g.fixed_work == fixed_work &&
            g.threads == threads && g.dense == dense && g.temporal == temporal && g.order == c->commit_order && g.views == c->views.get() && g.flags == c->flags.get() && g.stats == c->stats.get() && g.tile_list == tile_list &&
            memcmp(&g.kp, &c->kp, sizeof(c->kp)) == 0)
            return g.exec;
    if (c->iter_dev.reserve(1) != VM_OK) {
        c->use_graphs = 0;
        return nullptr;
    }
    const SweepLaunchers &SL = sweep_launchers(math_mode);
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        for (int it = 0; it < VM_GRAPH_ITERS; ++it) {
            for (int k = 0; k < 4; ++k) {
                SL.optimize(c->views.get(), n, cap, w, h, P, c->tables.get(), pass_offs[k][0], pass_offs[k][1], c->flags.get(), c->stats.get(), it, fixed_work, threads, c->iter_dev.get(), dense, tile_list, temporal, c->stream);
            }
        }
        SL.next_iter(c->iter_dev.get(), 0, VM_GRAPH_ITERS, c->stream);
        ok = hipStreamEndCapture(c->stream, &graph) == hipSuccess && graph;
    }
    if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) hipGraphDestroy(graph);
    (void)hipGetLastError();
    if (!ok) {
        c->use_graphs = 0;
        return nullptr;
    }
    if (c->graphs.size() >= 64) { // plenty for a pyramid's levels; start over rather than grow
        for (auto &g : c->graphs) hipGraphExecDestroy(g.exec);
        c->graphs.clear();
    }
    c->graphs.push_back({math_mode, n, w, h, cap, fixed_work, threads, dense, c->commit_order, temporal, c->views.get(), c->flags.get(), c->stats.get(), tile_list, c->kp, exec});
    return exec;
}

// The PASS token of a device.  k_pass spins at tile-local barriers, so the workgroups of all its tile
// groups must become co-resident; two PASS launches at once -- of two contexts, or of two PROCESSES
// sharing the device -- could hold part of the compute units each and starve each other's groups.  One
// holder at a time: inside the process a mutex per device, across processes an advisory flock() on a lock
// file named after the device's PCI bus id (so that HIP_VISIBLE_DEVICES renumbering cannot split it);
// whoever does not get the token runs STEP for that call.  Kernels that do not spin (every other
// schedule, any other program) only delay a PASS launch: they finish and free their compute units.
// VM_LOCK_DIR (default /tmp) holds the files; if one cannot be opened or locked the PASS schedule stays off in this
// process (STEP instead); the bounded barrier wait + the STEP rerun below remain the safety net for everything else.
namespace {
struct PassDevice {
    std::mutex mu;
    int fd = -2; // -2: not opened yet, -3: no usable lock file (PASS stays off in this process), >= 0: the lock file
};
PassDevice g_pass_dev[64];

struct PassToken {
    PassDevice *d = nullptr;
    bool owns = false;
    bool try_acquire(int device)
    {
        d = &g_pass_dev[device & 63];
        if (!d->mu.try_lock()) return false;
        if (d->fd == -2) {
            char bus[64] = "";
            if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) {
                (void)hipGetLastError();
                snprintf(bus, sizeof(bus), "ordinal%d", device);
            }
            for (char *q = bus; *q; ++q)
                if (*q == ':' || *q == '/' || *q == '.') *q = '_';
            const char *dir = getenv("VM_LOCK_DIR");
            const std::string path = std::string(dir && *dir ? dir : "/tmp") + "/vmorph-pass-" + bus + ".lock";
            // Open an existing file first: with fs.protected_regular (the default of many distributions) another
            // user's O_CREAT open of an existing file in a sticky directory fails with EACCES although a plain open
            // succeeds.  Create it only if it is not there (world-readable is all flock() needs).
            d->fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
            if (d->fd < 0 && errno == ENOENT) {
                d->fd = open(path.c_str(), O_RDONLY | O_CREAT | O_CLOEXEC, 0666);
                if (d->fd >= 0) (void)fchmod(d->fd, 0666); // readable by every user of the device whatever this process' umask
            }
            if (d->fd < 0) {
                // no lock file: exclusivity across processes cannot be had.  Refuse PASS rather than run it on a
                // process-local token -- two processes in PASS at once time out against each other (STEP is the
                // schedule of whoever does not hold the token anyway).  Said once.
                d->fd = -3;
                fprintf(stderr, "vmorph: cannot open %s (%s): the PASS schedule stays off on this device in this process; "
                                "set VM_LOCK_DIR to a directory every user of the device can read\n", path.c_str(), strerror(errno));
            }
        }
        if (d->fd == -3) {
            d->mu.unlock();
            return false;
        }
        if (d->fd >= 0) {
            int rc;
            do rc = flock(d->fd, LOCK_EX | LOCK_NB); while (rc != 0 && errno == EINTR);
            if (rc != 0) {
                if (errno != EWOULDBLOCK && errno != ENOLCK && errno != EOPNOTSUPP && errno != EINVAL) {
                    d->mu.unlock();                 // an error that says nothing about the holder: not this time
                    return false;
                }
                if (errno == EWOULDBLOCK) {         // another process holds the device's token
                    d->mu.unlock();
                    return false;
                }
                close(d->fd);                       // a file system without flock(): same as no lock file
                d->fd = -3;
                d->mu.unlock();
                return false;
            }
        }
        owns = true;
        return true;
    }
    void release()
    {
        if (!owns) return;
        if (d->fd >= 0) (void)flock(d->fd, LOCK_UN);
        d->mu.unlock();
        owns = false;
    }
    ~PassToken() { release(); }
};

// One call of vm_optimize_levels: what it was asked, what holds for the whole call, and what the batches add up to.
struct SweepRun {
    vm_ctx *c = nullptr;
    vm_level **lv = nullptr;
    int n = 0, w = 0, h = 0, cap = 1, fixed_work = 0;
    int temporal = 1; // the sweep variant of every launch of the call: 1 the general kernels, 0 the ones compiled without the temporal term
    size_t rec_bytes = 0; // of a level's record tags
    hipStream_t s = nullptr;
    VmKParams P{};
    const SweepLaunchers *SL = nullptr;
    SweepLevelPlan plan;
    SmallDensePresence small_dense; // this call's share of the small-level dense workgroups on the device, while it lasts
    PassToken pass_token;
    bool may_pass = false;   // PASS is wanted, fits the device, and this call holds the device's token
    bool pass_guard = false; // AUTO only: the levels as they stand before a PASS batch are kept, to rerun it with STEP should a barrier time out
    // the batch in hand
    int nb = 0;
    SweepBatchPlan b;
    int launches_before = 0;
    bool all_stopped = false;
    // the call so far
    int done = 0, launches = 0;
    double cand_prev = 1e9;  // line searches per iteration in the previous batch (first batch: dense)
    double tiles_prev = 1e9; // active tile visits per iteration and pair in the previous batch
    float ms = 0;
    float sched_ms[5] = {0, 0, 0, 0, 0}; // indexed by SweepSched
    int sched_launches[5] = {0, 0, 0, 0, 0};
    double clk_shader[2] = {0, 0}, clk_wall[2] = {0, 0}; // in-kernel clock probe: [0] dense TILE kernel, [1] k_pass
    std::vector<int> executed, improving, stopped, live;
    std::vector<double> st_tiles, st_cand, st_commit, st_eval;
};
} // namespace

// PASS admission: the level must be addressable by k_pass, a 256-workgroup chunk must fit the device, and the
// device's token must be free; then the error word and (AUTO) the snapshot buffer.
static int admit_pass(SweepRun &r)
{
    vm_ctx *c = r.c;
    vm_level &l0 = *r.lv[0];
    bool want_pass = r.plan.want_pass;
    // k_pass addresses a level's arrays by 32-bit byte offsets from its slab and from its schedule
    // workspace (72 + 104 B per pixel)
    if ((size_t)l0.rs * l0.h * 128 >= ((size_t)1 << 32)) {
        if (c->sweep_mode == VM_SWEEP_PASS)
            return vm_fail(VM_E_STATE, "vm_optimize_level: the PASS schedule addresses levels of up to 32 Mpixel");
        want_pass = false;
    }
    if (want_pass) { // a 256-workgroup chunk of the launch must fit the device at once
        int &res = c->pass_resident[(c->math_mode & 7) * 2 + r.temporal];
        if (res < 0) res = r.SL->pass_resident(c->device, r.temporal);
        if (res < 256) {
            if (c->sweep_mode == VM_SWEEP_PASS)
                return vm_fail(VM_E_STATE, "vm_optimize_level: the PASS schedule needs 256 co-resident workgroups, this device holds %d", res);
            want_pass = false;
        }
    }
    if (want_pass && r.pass_token.try_acquire(c->device) && !c->pass_err_host.get()) { // the error word and its mirror: made together, the mirror last
        if (int rc = c->pass_err.reserve(64)) return rc;
        VM_HIP(hipMemsetAsync(c->pass_err.get(), 0, 256, r.s));
        if (int rc = c->pass_err_host.reserve(64)) return rc;
    }
    r.may_pass = want_pass && r.pass_token.owns;
    r.pass_guard = r.may_pass && c->sweep_mode == VM_SWEEP_AUTO;
    if (r.pass_guard) {
        size_t need = 0;
        for (int i = 0; i < r.n; ++i) need += r.lv[i]->slab.capacity();
        if (int rc = c->pass_snap.reserve(need)) return rc;
    }
    return VM_OK;
}

// Buffers, workspaces and the level views of the call on the device; flags, counters and records start from zero.
static int prepare(SweepRun &r)
{
    vm_ctx *c = r.c;
    const int n = r.n;
    hipStream_t s = r.s;
    vm_level &l0 = *r.lv[0];
    const size_t words = (size_t)r.cap * n;
    if (int rc = c->flags.reserve(words)) return rc;
    if (int rc = c->flags_host.reserve(words)) return rc;
    if (int rc = c->stats.reserve(words * VM_STAT_WORDS)) return rc;
    if (int rc = c->stats_host.reserve(words * VM_STAT_WORDS)) return rc;
    if (int rc = c->views.reserve(n)) return rc;
    // levels that may run the SPLIT / STEP schedules need their workspace before the views
    // are copied to the device
    if (r.plan.needs_ws)
        for (int i = 0; i < n; ++i)
            if (int rc = level_ensure_ws(c, *r.lv[i])) return rc;
    if (r.plan.may_sparse)
        for (int i = 0; i < n; ++i) {
            if (int rc = level_ensure_sparse(c, *r.lv[i])) return rc;
            // the stamps are epochs of THIS call (iteration * 4 + pass + 1)
            VM_HIP(hipMemsetAsync(r.lv[i]->view.sp_stamp, 0, (size_t)l0.imp_rs * l0.imp_rows * 4, s));
        }
    {
        std::vector<VmLevelView> hv(n);
        for (int i = 0; i < n; ++i) hv[i] = r.lv[i]->view;
        VM_HIP(hipMemcpyAsync(c->views.get(), hv.data(), (size_t)n * sizeof(VmLevelView), hipMemcpyHostToDevice, s));
        VM_HIP(hipStreamSynchronize(s)); // hv is a stack object
    }
    VM_HIP(hipMemsetAsync(c->flags.get(), 0, words * 4, s));
    VM_HIP(hipMemsetAsync(c->stats.get(), 0, words * 4 * VM_STAT_WORDS, s));
    if (r.plan.listed_ok) {
        const size_t entries = (size_t)r.plan.tiles * n;
        const size_t need = 4 * (size_t)r.cap + 2 * entries; // counters per iteration and pass, stamps, entries
        if (int rc = c->tile_list.reserve(need, s)) return rc;
        VM_HIP(hipMemsetAsync(c->tile_list.get(), 0, (4 * (size_t)r.cap + entries) * sizeof(uint32_t), s));
    }
    if (r.plan.needs_ws) // epochs restart with every call: forget old records
        for (int i = 0; i < n; ++i) {
            VM_HIP(hipMemsetAsync(r.lv[i]->view.rec_tag, 0, r.rec_bytes, s));
            VM_HIP(hipMemsetAsync(r.lv[i]->view.rec_tag2, 0, r.rec_bytes, s));
        }
    r.executed.assign(n, r.cap);
    r.improving.assign(n, 1);
    r.stopped.assign(n, 0);
    r.live.assign(n, -1);
    r.st_tiles.assign(n, 0.0);
    r.st_cand.assign(n, 0.0);
    r.st_commit.assign(n, 0.0);
    r.st_eval.assign(n, 0.0);
    return admit_pass(r);
}

static int enqueue_sparse(SweepRun &r)
{
    vm_ctx *c = r.c;
    for (int i = 0; i < r.n; ++i)
        VM_HIP(hipMemsetAsync(r.lv[i]->view.sp_cnt, 0, 8, r.s));
    // (forced SPARSE schedule with parts given: the LDS capacity of the word list, 0 < parts; parts = 1 is
    // "as good as none": the list then lives in memory from the first pass it holds two words -- tests)
    r.SL->sparse(
        c->views.get(), r.n, r.cap, r.w, r.h, r.P, c->tables.get(), c->flags.get(), c->stats.get(), r.done, r.nb, r.fixed_work, r.plan.threads, r.b.dense,
        c->sweep_mode == VM_SWEEP_SPARSE && c->sweep_parts > 0 ? c->sweep_parts : 1 << 20, c->sparse_resident, r.temporal, r.s);
    r.launches += 2;
    r.small_dense.leave();
    return VM_OK;
}

// TILE: whole groups of VM_GRAPH_ITERS iterations are graph replays, the rest eager launches
static int enqueue_tile(SweepRun &r)
{
    vm_ctx *c = r.c;
    if (r.b.small_dense)
        r.small_dense.enter(c->device, r.plan.groups);
    else
        r.small_dense.leave();
    const int tile_threads = r.small_dense.in_flight() >= r.plan.corun_min_wgs ? 256 : r.plan.threads;
    uint32_t *const tile_list = r.b.use_tile_list ? c->tile_list.get() : nullptr;
    const int form = r.b.tile_form();
    const int end = r.done + r.nb;
    int it0 = r.done;
    if (r.nb >= VM_GRAPH_ITERS) {
        if (hipGraphExec_t ge = sweep_graph(c, c->math_mode, r.n, r.w, r.h, r.cap, r.fixed_work, tile_threads, form, tile_list, r.temporal, r.P)) {
            r.SL->next_iter(c->iter_dev.get(), 1, r.done, r.s);
            for (; it0 + VM_GRAPH_ITERS <= end; it0 += VM_GRAPH_ITERS) {
                VM_HIP(hipGraphLaunch(ge, r.s));
                r.launches += 4 * VM_GRAPH_ITERS;
            }
        }
    }
    for (int it = it0; it < end; ++it)
        for (int k = 0; k < 4; ++k) {
            r.SL->optimize(c->views.get(), r.n, r.cap, r.w, r.h, r.P, c->tables.get(), pass_offs[k][0], pass_offs[k][1], c->flags.get(), c->stats.get(), it, r.fixed_work, tile_threads, nullptr, form, tile_list, r.temporal, r.s);
            ++r.launches;
        }
    return VM_OK;
}

// the two-kernel SPLIT (forced only)
static int enqueue_split(SweepRun &r)
{
    vm_ctx *c = r.c;
    r.small_dense.leave();
    for (int it = r.done; it < r.done + r.nb; ++it)
        for (int k = 0; k < 4; ++k) {
            r.SL->split(c->views.get(), r.n, r.cap, r.w, r.h, r.P, c->tables.get(), pass_offs[k][0], pass_offs[k][1], k, c->flags.get(), c->stats.get(), it, r.fixed_work, r.plan.threads, r.plan.parts, r.temporal, r.s);
            r.launches += 8;
        }
    return VM_OK;
}

// per-workgroup count slots of the last two launches (k_step / k_pass fold them one launch late): the two halves of
// step_slots, `need` words each
static int reserve_slots(SweepRun &r, size_t need, uint32_t *slots[2])
{
    if (int rc = r.c->step_slots.reserve(2 * need, r.s)) return rc;
    slots[0] = r.c->step_slots.get();
    slots[1] = r.c->step_slots.get() + r.c->step_slots.capacity() / 2;
    return VM_OK;
}

// STEP: one launch per phase, the commit of a phase in the launch of the next; a closing launch folds the last
static int enqueue_step(SweepRun &r)
{
    vm_ctx *c = r.c;
    const int threads = r.plan.threads, parts = r.plan.parts;
    uint32_t *slots[2];
    if (int rc = reserve_slots(r, (size_t)r.plan.tiles * parts * r.n * 4, slots)) return rc;
    r.small_dense.leave();
    uint32_t last_epoch = 0;
    int sb = 0;         // step index inside this batch: parity = which copy of the sums is read
    int slot_iter = -1; // iteration whose counts the previous launch left in its slots
    for (int it = r.done; it < r.done + r.nb; ++it)
        for (int k = 0; k < 4; ++k) {
            for (int ph = 0; ph < 4; ++ph, ++sb) {
                const uint32_t epoch = 1u + (uint32_t)((it * 4 + k) * 4 + ph);
                r.SL->step(
                    c->views.get(), r.n, r.cap, r.w, r.h, r.P, c->tables.get(), pass_offs[k][0], pass_offs[k][1], ph >> 1, ph & 1, epoch,
                    sb == 0 ? 0u : epoch - 1u, sb & 1, 1, c->flags.get(), c->stats.get(), it, r.fixed_work, threads, parts,
                    slots[sb & 1], slots[(sb + 1) & 1], sb == 0 ? -1 : slot_iter, r.temporal, r.s);
                slot_iter = it;
                last_epoch = epoch;
            }
            r.launches += 4;
        }
    // fold the last phase's records in place: copy 0 is complete again
    r.SL->step(
        c->views.get(), r.n, r.cap, r.w, r.h, r.P, c->tables.get(), 0, 0, 0, 0, 0u, last_epoch, 2, 0, c->flags.get(), c->stats.get(),
        r.done + r.nb - 1, r.fixed_work, threads, parts, slots[sb & 1], slots[(sb + 1) & 1], sb == 0 ? -1 : slot_iter, r.temporal, r.s);
    ++r.launches;
    return VM_OK;
}

// PASS: one launch per pass, then a tail launch for the counts the last one left in its slots
static int enqueue_pass(SweepRun &r)
{
    vm_ctx *c = r.c;
    const int pass_groups = r.plan.groups, pass_blocks = (pass_groups + 7) / 8 * 256;
    if (r.pass_guard) {
        size_t off = 0;
        for (int i = 0; i < r.n; ++i) {
            VM_HIP(hipMemcpyAsync(c->pass_snap.get() + off, r.lv[i]->slab.get(), r.lv[i]->slab.capacity(), hipMemcpyDeviceToDevice, r.s));
            off += r.lv[i]->slab.capacity();
        }
    }
    // barrier counters of every launch of the batch, zeroed once
    const size_t need_bar = (size_t)r.nb * 4 * pass_groups * VM_PASS_SYNC_WORDS;
    if (int rc = c->pass_bar.reserve(std::max(need_bar, (size_t)64 * 4 * 8 * VM_PASS_SYNC_WORDS), r.s)) return rc;
    VM_HIP(hipMemsetAsync(c->pass_bar.get(), 0, need_bar * sizeof(uint32_t), r.s));
    uint32_t *slots[2];
    if (int rc = reserve_slots(r, (size_t)pass_blocks * 4, slots)) return rc;
    r.small_dense.leave();
    const int pass_switches = r.plan.pass_switches;
    int sb = 0, slot_iter = -1; // as in enqueue_step
    for (int it = r.done; it < r.done + r.nb; ++it)
        for (int k = 0; k < 4; ++k) {
            r.SL->pass(
                c->views.get(), r.n, r.cap, r.w, r.h, r.P, c->tables.get(), pass_offs[k][0], pass_offs[k][1], 1u + (uint32_t)((it * 4 + k) * 4),
                c->pass_bar.get() + (size_t)((it - r.done) * 4 + k) * pass_groups * VM_PASS_SYNC_WORDS, c->flags.get(), c->stats.get(), it, r.fixed_work,
                slots[sb & 1], slots[(sb + 1) & 1], sb == 0 ? -1 : slot_iter, c->pass_err.get(),
                c->pass_dbg.get(), 1, pass_switches, r.temporal, r.s);
            slot_iter = it;
            ++sb;
            ++r.launches;
        }
    if (sb > 0) {
        r.SL->pass(
            c->views.get(), r.n, r.cap, r.w, r.h, r.P, c->tables.get(), 0, 0, 0u, nullptr, c->flags.get(), c->stats.get(), r.done + r.nb - 1, r.fixed_work,
            nullptr, slots[(sb + 1) & 1], slot_iter, c->pass_err.get(), nullptr, 0, pass_switches, r.temporal, r.s);
        ++r.launches;
    }
    return VM_OK;
}

// The sweep launches of the batch in hand under its schedule, bracketed by the context's HIP events.
static int enqueue_batch(SweepRun &r)
{
    vm_ctx *c = r.c;
    r.launches_before = r.launches;
    VM_HIP(hipEventRecord(c->ev0.get(), r.s));
    int rc = VM_OK;
    switch (r.b.sched) {
    case SCHED_SPARSE: rc = enqueue_sparse(r); break;
    case SCHED_PASS: rc = enqueue_pass(r); break;
    case SCHED_STEP: rc = r.b.step ? enqueue_step(r) : enqueue_split(r); break;
    default: rc = enqueue_tile(r); break;
    }
    if (rc != VM_OK) return rc;
    VM_HIP(hipEventRecord(c->ev1.get(), r.s));
    VM_HIP(hipGetLastError());
    return VM_OK;
}

// the batch's flags and counters (and the PASS error word) on the host; waits for the batch
static int read_back(SweepRun &r)
{
    vm_ctx *c = r.c;
    const int cap = r.cap, done = r.done, nb = r.nb;
    if (r.b.sched == SCHED_PASS)
        VM_HIP(hipMemcpyAsync(c->pass_err_host.get(), c->pass_err.get(), 4, hipMemcpyDeviceToHost, r.s));
    // (one strided copy per array instead of 2 n small ones was measured: 60 pairs 838 -> 836 ms, 8 pairs 328 -> 332: not kept)
    for (int i = 0; i < r.n; ++i) {
        VM_HIP(hipMemcpyAsync(c->flags_host.get() + (size_t)i * cap + done, c->flags.get() + (size_t)i * cap + done, (size_t)nb * 4, hipMemcpyDeviceToHost, r.s));
        VM_HIP(hipMemcpyAsync(c->stats_host.get() + ((size_t)i * cap + done) * VM_STAT_WORDS, c->stats.get() + ((size_t)i * cap + done) * VM_STAT_WORDS,
                              (size_t)nb * 4 * VM_STAT_WORDS, hipMemcpyDeviceToHost, r.s));
    }
    VM_HIP(hipStreamSynchronize(r.s));
    return VM_OK;
}

// A tile barrier of the PASS batch in hand timed out.  Forced PASS: an error.  AUTO: the batch never happened --
// state, records, flags and counters as before it -- the caller runs it again, with STEP, and this context stays off
// PASS from now on.
static int recover_pass_timeout(SweepRun &r)
{
    vm_ctx *c = r.c;
    const int cap = r.cap, done = r.done, nb = r.nb;
    VM_HIP(hipMemsetAsync(c->pass_err.get(), 0, 4, r.s));
    if (!r.pass_guard)
        return vm_fail(VM_E_DEVICE, "vm_optimize_level: a tile barrier of the PASS schedule timed out (are all of this device's "
                                    "compute units available to this process?  VM_SWEEP_AUTO falls back to the STEP schedule by itself)");
    size_t off = 0;
    for (int i = 0; i < r.n; ++i) {
        VM_HIP(hipMemcpyAsync(r.lv[i]->slab.get(), c->pass_snap.get() + off, r.lv[i]->slab.capacity(), hipMemcpyDeviceToDevice, r.s));
        off += r.lv[i]->slab.capacity();
        VM_HIP(hipMemsetAsync(r.lv[i]->view.rec_tag, 0, r.rec_bytes, r.s));
        VM_HIP(hipMemsetAsync(r.lv[i]->view.rec_tag2, 0, r.rec_bytes, r.s));
        VM_HIP(hipMemsetAsync(c->flags.get() + (size_t)i * cap + done, 0, (size_t)nb * 4, r.s));
        VM_HIP(hipMemsetAsync(c->stats.get() + ((size_t)i * cap + done) * VM_STAT_WORDS, 0, (size_t)nb * 4 * VM_STAT_WORDS, r.s));
    }
    r.launches = r.launches_before;
    r.may_pass = false;
    if (!c->pass_latched_off) c->pass_latched_by_test = c->pass_test_timeout != 0;
    c->pass_latched_off = true;
    ++c->pass_fallbacks;
    r.pass_token.release();
    return VM_OK;
}

// The batch in hand is over: its time, and its flags and counters per pair -- who stopped, and what the next batch's
// schedule goes by.
static int fold_stats(SweepRun &r)
{
    vm_ctx *c = r.c;
    const int cap = r.cap, done = r.done, nb = r.nb, sched = r.b.sched;
    float bms = 0;
    VM_HIP(hipEventElapsedTime(&bms, c->ev0.get(), c->ev1.get()));
    r.ms += bms;
    r.sched_ms[sched] += bms;
    r.sched_launches[sched] += r.launches - r.launches_before;
    r.all_stopped = true;
    double b_cand = 0, b_tiles = 0;
    for (int i = 0; i < r.n; ++i) {
        const uint32_t *fl = c->flags_host.get() + (size_t)i * cap, *st = c->stats_host.get() + (size_t)i * cap * VM_STAT_WORDS;
        for (int it = done; it < done + nb && !r.stopped[i]; ++it) {
            // [0] tile visits (TILE schedule), [3] tile-phases with records (SPLIT schedule)
            r.st_tiles[i] += st[VM_STAT_WORDS * it] + 0.25 * st[VM_STAT_WORDS * it + 3];
            b_tiles += st[VM_STAT_WORDS * it] + 0.25 * st[VM_STAT_WORDS * it + 3];
            r.st_cand[i] += st[VM_STAT_WORDS * it + 1];
            b_cand += st[VM_STAT_WORDS * it + 1];
            r.st_commit[i] += st[VM_STAT_WORDS * it + 2];
            r.st_eval[i] += st[VM_STAT_WORDS * it + 4];
            c->sparse_resident_visits += st[VM_STAT_WORDS * it + 5];
            if (i == 0 && (sched == SCHED_TILE_DENSE || sched == SCHED_PASS)) { // in-kernel clock probe of the dense TILE kernel / of k_pass (pair 0 only)
                r.clk_shader[sched == SCHED_PASS] += st[VM_STAT_WORDS * it + 6];
                r.clk_wall[sched == SCHED_PASS] += st[VM_STAT_WORDS * it + 7];
            }
            r.improving[i] = fl[it] != 0;
            if (!r.improving[i] && r.live[i] < 0) r.live[i] = it + 1; // the reference's loop ends here (morph.cu:1390)
            if (!r.improving[i] && !r.fixed_work) { r.executed[i] = it + 1; r.stopped[i] = 1; }
        }
        r.all_stopped = r.all_stopped && r.stopped[i];
    }
    r.cand_prev = b_cand / nb;
    r.tiles_prev = b_tiles / nb / r.n;
    r.done += nb;
    return VM_OK;
}

static void report(const SweepRun &r, vm_progress *out)
{
    for (int i = 0; i < r.n && out; ++i) {
        out[i].iters = r.executed[i];
        out[i].iters_live = r.live[i] < 0 ? r.executed[i] : std::min(r.live[i], r.executed[i]);
        out[i].improving = r.improving[i];
        out[i].pixel_iters = (double)r.executed[i] * r.w * r.h;
        out[i].elapsed_ms = r.ms;       // of the batch the pair was solved in
        out[i].launches = r.launches;   // idem
        out[i].active_tiles = r.st_tiles[i];
        out[i].candidates = r.st_cand[i];
        out[i].commits = r.st_commit[i];
        out[i].evaluations = r.st_eval[i];
        for (int k = 0; k < 5; ++k) { // of the batch, like elapsed_ms
            out[i].sched_ms[k] = r.sched_ms[k];
            out[i].sched_launches[k] = r.sched_launches[k];
        }
        for (int k = 0; k < 2; ++k) {
            out[i].clk_shader_ticks[k] = r.clk_shader[k];
            out[i].clk_wall_ticks[k] = r.clk_wall[k];
        }
    }
}

// The iteration count of `do { ... iter++; } while (iter < _max_iter && ...)` (morph.cu:1378-1390)
// for the float _max_iter of morph.h:20: max(1, ceil(max_iter)).  Not finite, or beyond 2^20
// iterations, is a caller error (the flag and counter arrays are sized by it).
int vm_iteration_cap(float max_iter, int *cap)
{
    if (!std::isfinite(max_iter)) return vm_fail(VM_E_INVALID, "max_iter must be finite (got %g)", (double)max_iter);
    if (max_iter > (float)(1 << 20)) return vm_fail(VM_E_INVALID, "max_iter %g exceeds the limit of %d iterations per level", (double)max_iter, 1 << 20);
    *cap = std::max(1, (int)std::ceil(max_iter));
    return VM_OK;
}

// The same level (one page) of n frame pairs -- or n pages of a video that do not depend on
// each other -- relaxed by the same launches.
int vm_optimize_levels(vm_ctx *c, vm_level **lv, int n, float max_iter, volatile const int *run_flag,
                       int fixed_work, vm_progress *out)
{
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    VM_ON_DEVICE(c);
    vm_level &l0 = *lv[0];
    for (int i = 0; i < n; ++i) {
        vm_level &l = *lv[i];
        if (l.w != l0.w || l.h != l0.h) return vm_fail(VM_E_INVALID, "batch: pyramids must share their geometry");
        if (!l.has_state) return vm_fail(VM_E_STATE, "vm_optimize_level: level not initialised");
        if ((l.view.temp_mask != nullptr) != (l0.view.temp_mask != nullptr))
            return vm_fail(VM_E_INVALID, "batch: pages with and without the temporal term cannot share a launch");
    }
    SweepRun r;
    r.c = c;
    r.lv = lv;
    r.n = n;
    r.w = l0.w;
    r.h = l0.h;
    r.fixed_work = fixed_work;
    // uniform over the batch by the check above; vm_dbg_sweep_variant 1 keeps the general kernels
    r.temporal = l0.view.temp_mask != nullptr || c->sweep_variant == 1;
    r.rec_bytes = (size_t)l0.rs * l0.h * 4;
    r.s = c->stream;
    r.P = {c->kp.w_ui, c->kp.w_tps, c->kp.w_ssim, c->kp.ssim_clamp, c->kp.eps, c->kp.bcond, c->kp.w_temp, c->commit_order};
    if (int rc = vm_iteration_cap(max_iter, &r.cap)) return rc;
    r.SL = &sweep_launchers(c->math_mode);
    const SweepCall call{l0.w, l0.h, n, c->math_mode, c->sweep_mode, c->sweep_threads, c->sweep_parts,
                         c->pass_latched_off, c->pass_test_timeout != 0};
    r.plan = plan_level(call, SweepSwitches::from_environment());
    if (int rc = prepare(r)) return rc;
    // Iterations are enqueued in batches; each sweep kernel of iteration i exits at once (per
    // pair) when iteration i-1 did not improve (device-side flag), so running past convergence
    // inside a batch costs launch latency only, and the host reads the flags once per batch
    // instead of once per iteration.
    bool cancelled = false;
    int batch = 2; // a short first batch: the schedule of the rest depends on what it finds
    while (r.done < r.cap) {
        r.nb = std::min(batch, r.cap - r.done);
        r.b = plan_batch(r.plan, r.cand_prev, r.tiles_prev, r.may_pass);
        if (int rc = enqueue_batch(r)) return rc;
        if (int rc = read_back(r)) return rc;
        if (r.b.sched == SCHED_PASS && c->pass_err_host.get()[0]) {
            if (int rc = recover_pass_timeout(r)) return rc;
            continue;
        }
        if (int rc = fold_stats(r)) return rc;
        if (r.all_stopped) break;
        if (run_flag && !*run_flag) {
            for (int i = 0; i < n; ++i) if (!r.stopped[i]) r.executed[i] = r.done;
            cancelled = true;
            break;
        }
        batch = std::min(batch * 4, 64);
    }
    // everything this call wrote into the levels is enqueued: consumers on other streams wait on this event
    // (vm_frame_set_v_from_level across contexts) instead of draining this stream from the host
    VM_HIP(hipEventRecord(c->done_ev.get(), r.s));
    report(r, out);
    return cancelled ? vm_fail(VM_E_CANCELLED, "vm_optimize_level: cancelled by run_flag") : VM_OK;
}
