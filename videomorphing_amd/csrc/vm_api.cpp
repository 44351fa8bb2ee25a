// vm_api.cpp -- implementation of the C-ABI declared in include/vmorph.h:
// contexts, pyramids, host<->device copies, the host-side coarse solve and the
// coarse-to-fine driver.  The sweep of one level (vm_optimize_levels: which
// schedule, the launches, the counters) is vm_sweep_sched.cpp over the policy of
// vm_sweep_plan.h.  Kernels live in vm_morph_kernels.hip (optimizer),
// vm_render.hip (compositor) and vm_poisson.hip (boundary extension).
#include "vm_internal.h"
#include "vm_host.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;

int vm_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *vm_last_error(void) { return g_err.c_str(); }
extern "C" const char *vm_version(void) { return "vmorph-mi355x 0.1 (gfx950)"; }

// ---------------------------------------------------------------------------
// constant tables (thin-plate stencil per border class, improving-mask window
// bits).  Product-side generator: the stencil row of a pixel is the Hessian
// row of the discrete bending energy  sum (dxx v)^2 + (dyy v)^2 + 2 (dxy v)^2
// over all operator placements that fit in the image -- what
// Algorithm/stencils.cpp:156-261 tabulates per border class.
static void build_tables(uint32_t *tab)
{
    float tps[5][5][5][5];
    memset(tps, 0, sizeof(tps));
    // a 5x5 image realises every border class pair once: pixel (n,m) has class (m,n)
    const int N = 5;
    struct Op { int n; int dx[4], dy[4]; float c[4]; float w; };
    const Op ops[3] = {
        {3, {-1, 0, 1, 0}, {0, 0, 0, 0}, {1, -2, 1, 0}, 1.0f},  // dxx, centred
        {3, {0, 0, 0, 0}, {-1, 0, 1, 0}, {1, -2, 1, 0}, 1.0f},  // dyy, centred
        {4, {0, 1, 0, 1}, {0, 0, 1, 1}, {1, -1, -1, 1}, 2.0f},  // dxy on the cell (x..x+1, y..y+1)
    };
    for (int k = 0; k < 3; ++k)
        for (int cy = 0; cy < N; ++cy)
            for (int cx = 0; cx < N; ++cx) {
                const Op &o = ops[k];
                bool fits = true;
                for (int t = 0; t < o.n; ++t) {
                    int x = cx + o.dx[t], y = cy + o.dy[t];
                    if (x < 0 || x >= N || y < 0 || y >= N) fits = false;
                }
                if (!fits) continue;
                // d/dv_p of w*(sum c_t v_t)^2 = 2 w c_p sum c_t v_t
                for (int p = 0; p < o.n; ++p)
                    for (int t = 0; t < o.n; ++t) {
                        int px = cx + o.dx[p], py = cy + o.dy[p];
                        int qx = cx + o.dx[t], qy = cy + o.dy[t];
                        tps[py][px][qy - py + 2][qx - px + 2] += 2.0f * o.w * o.c[p] * o.c[t];
                    }
            }
    for (int i = 0; i < 625; ++i) {
        float f = (&tps[0][0][0][0])[i];
        memcpy(&tab[VM_TAB_TPS + i], &f, 4);
    }
    // improving-mask bits (stencils.cpp:90-126): for a pixel at (ox,oy) inside
    // its 5x5 block, which bits of the 3x3 neighbouring blocks fall in its window
    for (int oy = 0; oy < 5; ++oy)
        for (int ox = 0; ox < 5; ++ox)
            for (int by = 0; by < 3; ++by)
                for (int bx = 0; bx < 3; ++bx) {
                    uint32_t m = 0;
                    for (int ry = 0; ry < 5; ++ry)
                        for (int rx = 0; rx < 5; ++rx) {
                            int wx = (bx - 1) * 5 + rx - ox, wy = (by - 1) * 5 + ry - oy;
                            if (wx >= -2 && wx <= 2 && wy >= -2 && wy <= 2)
                                m |= 1u << (rx + ry * 5);
                        }
                    tab[VM_TAB_IMP + ((oy * 5 + ox) * 3 + by) * 3 + bx] = m;
                }
}

// ---------------------------------------------------------------------------
static void ctx_free(vm_ctx *c);

// Live contexts.  Destroying a pyramid, video, frame or sync object after its context is a caller
// error; a garbage-collected host language can produce that order.  vm_destroy_object (vm_host.h)
// checks here and then frees the object's device buffers without the context (every object
// remembers its device; hipFree needs neither the stream nor the context, after a device-wide
// synchronise nothing can still be using them): no use-after-free and no leak.  Every other entry
// point refuses an object whose context is gone.
#include <set>
static std::mutex g_live_mu;
static std::set<const vm_ctx *> g_live;
bool vm_ctx_alive(const vm_ctx *c)
{
    std::lock_guard<std::mutex> lock(g_live_mu);
    return g_live.count(c) != 0;
}

extern "C" int vm_ctx_create(int device, vm_ctx **out)
{
    if (!out) return vm_fail(VM_E_INVALID, "vm_ctx_create: out is NULL");
    *out = nullptr;
    // VM_REDUCTION=ordered|atomic: the reduction mode the context starts with (vm_set_reduction), for drivers that do not call it
    int reduction = VM_REDUCE_ATOMIC;
    if (const char *e = getenv("VM_REDUCTION")) {
        if (!strcmp(e, "ordered")) reduction = VM_REDUCE_ORDERED;
        else if (strcmp(e, "atomic")) return vm_fail(VM_E_INVALID, "vm_ctx_create: VM_REDUCTION=%s (ordered or atomic)", e);
    }
    // VM_SWEEP_VARIANT=general|level (development): the sweep variant the context starts with (vm_dbg_sweep_variant), to
    // time the two variants against each other inside one library
    int sweep_variant = 0;
    if (const char *e = getenv("VM_SWEEP_VARIANT")) {
        if (!strcmp(e, "general")) sweep_variant = 1;
        else if (strcmp(e, "level")) return vm_fail(VM_E_INVALID, "vm_ctx_create: VM_SWEEP_VARIANT=%s (general or level)", e);
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return vm_fail(VM_E_DEVICE, "vm_ctx_create: no HIP device (%s); there is no CPU fallback",
                       hipGetErrorString(e));
    if (device < 0 || device >= ndev)
        return vm_fail(VM_E_INVALID, "vm_ctx_create: device %d out of range (0..%d)", device, ndev - 1);
    vm_ctx *c = new vm_ctx();
    c->device = device;
    c->reduction = reduction;
    c->sweep_variant = sweep_variant;
    VM_ON_DEVICE(c);
    c->math_mode = VM_MATH_EXACT;
    c->kp = {10.0f, 1e5f, 0.05f, 100.0f, 0.0f, 0.01f, VM_BCOND_NONE}; // UI/MdiEditor.cpp:131-140
    // a context that cannot be completed is torn down again: nothing leaks on the error paths
    uint32_t tab[VM_TAB_WORDS];
    build_tables(tab);
    auto hip = [](hipError_t e) { return e == hipSuccess ? VM_OK : vm_fail(VM_E_DEVICE, "vm_ctx_create: %s", hipGetErrorString(e)); };
    int rc = hip(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (rc == VM_OK) rc = c->ev0.create();
    if (rc == VM_OK) rc = c->ev1.create();
    if (rc == VM_OK) rc = c->done_ev.create(hipEventDisableTiming);
    if (rc == VM_OK) rc = c->xfer_ev.create(hipEventDisableTiming);
    if (rc == VM_OK) rc = hip(hipEventRecord(c->done_ev.get(), c->stream));
    if (rc == VM_OK) rc = c->tables.reserve(VM_TAB_WORDS);
    if (rc == VM_OK) rc = hip(hipMemcpy(c->tables.get(), tab, sizeof(tab), hipMemcpyHostToDevice));
    if (rc == VM_OK) rc = c->flags.reserve(4096);
    if (rc == VM_OK) rc = c->flags_host.reserve(4096);
    if (rc == VM_OK) rc = c->stats.reserve(4096 * VM_STAT_WORDS);
    if (rc == VM_OK) rc = c->stats_host.reserve(4096 * VM_STAT_WORDS);
    if (rc != VM_OK) {
        ctx_free(c);
        return rc;
    }
    {
        std::lock_guard<std::mutex> lock(g_live_mu);
        g_live.insert(c);
    }
    *out = c;
    return VM_OK;
}

static void ctx_free(vm_ctx *c)
{
    hipStream_t s = c->stream;
    if (s) hipStreamSynchronize(s);
    for (auto &g : c->graphs) hipGraphExecDestroy(g.exec);
    delete c;
    if (s) hipStreamDestroy(s);
    (void)hipGetLastError();
}

extern "C" void vm_ctx_destroy(vm_ctx *c)
{
    if (!c || !vm_ctx_alive(c)) return;
    {
        std::lock_guard<std::mutex> lock(g_live_mu);
        g_live.erase(c);
    }
    VM_ON_DEVICE_VOID(c);
    ctx_free(c);
}

extern "C" int vm_ctx_sync(vm_ctx *c)
{
    VM_ENTER(c);
    VM_HIP(hipStreamSynchronize(c->stream));
    return VM_OK;
}

extern "C" int vm_set_params(vm_ctx *c, const vm_kern_params *p)
{
    if (!c || !p) return vm_fail(VM_E_INVALID, "vm_set_params: NULL argument");
    if (p->bcond < VM_BCOND_NONE || p->bcond > VM_BCOND_BORDER)
        return vm_fail(VM_E_INVALID, "vm_set_params: bcond %d", p->bcond);
    if (!(p->eps > 0)) return vm_fail(VM_E_INVALID, "vm_set_params: eps must be > 0");
    c->kp = *p;
    return VM_OK;
}

extern "C" int vm_get_params(vm_ctx *c, vm_kern_params *p)
{
    if (!c || !p) return vm_fail(VM_E_INVALID, "vm_get_params: NULL argument");
    *p = c->kp;
    return VM_OK;
}

extern "C" int vm_set_math_mode(vm_ctx *c, int mode)
{
    if (!c || mode < VM_MATH_EXACT || mode > VM_MATH_REF_TEX8_TRUNC)
        return vm_fail(VM_E_INVALID, "vm_set_math_mode: bad argument");
    c->math_mode = mode;
    return VM_OK;
}

extern "C" int vm_set_commit_order(vm_ctx *c, int order)
{
    if (!c) return vm_fail(VM_E_INVALID, "vm_set_commit_order: ctx is NULL");
    if (order < 0 || order > 3) return vm_fail(VM_E_INVALID, "vm_set_commit_order: order %d (0 row-major, 1 reversed, 2 column-major, 3 column-major reversed)", order);
    c->commit_order = order;
    return VM_OK;
}

extern "C" int vm_set_reduction(vm_ctx *c, int mode)
{
    if (!c) return vm_fail(VM_E_INVALID, "vm_set_reduction: ctx is NULL");
    if (mode != VM_REDUCE_ATOMIC && mode != VM_REDUCE_ORDERED)
        return vm_fail(VM_E_INVALID, "vm_set_reduction: mode %d (0 atomic, 1 ordered)", mode);
    c->reduction = mode;
    return VM_OK;
}

extern "C" int vm_dbg_sparse_resident(vm_ctx *c, int mode)
{
    if (!c) return vm_fail(VM_E_INVALID, "vm_dbg_sparse_resident: ctx is NULL");
    if (mode < 0 || mode > 3) return vm_fail(VM_E_INVALID, "vm_dbg_sparse_resident: mode %d (0 automatic, 1 never, 2 re-centre at every commit, 3 give up at the first commit)", mode);
    c->sparse_resident = mode;
    return VM_OK;
}

extern "C" int vm_dbg_sweep_variant(vm_ctx *c, int mode)
{
    if (!c) return vm_fail(VM_E_INVALID, "vm_dbg_sweep_variant: ctx is NULL");
    if (mode < 0 || mode > 1) return vm_fail(VM_E_INVALID, "vm_dbg_sweep_variant: mode %d (0 by the level, 1 always the general kernels)", mode);
    c->sweep_variant = mode;
    return VM_OK;
}

extern "C" int vm_dbg_sparse_resident_visits(vm_ctx *c)
{
    if (!c) return vm_fail(VM_E_INVALID, "vm_dbg_sparse_resident_visits: ctx is NULL");
    return (int)std::min<unsigned long long>(c->sparse_resident_visits, 0x7fffffffull);
}

extern "C" int vm_dbg_pass_force_timeout(vm_ctx *c, int on)
{
    if (!c) return vm_fail(VM_E_INVALID, "vm_dbg_pass_force_timeout: ctx is NULL");
    c->pass_test_timeout = on ? 1 : 0;
    // switching the hook off re-admits the context to PASS only if the HOOK latched it off: a latch set by a
    // genuine barrier timeout (masked or shared compute units) stays
    if (!on && c->pass_latched_by_test) {
        c->pass_latched_off = false;
        c->pass_latched_by_test = false;
    }
    return VM_OK;
}

extern "C" int vm_dbg_pass_fallbacks(vm_ctx *c)
{
    return c ? c->pass_fallbacks : -1;
}

extern "C" int vm_dbg_pass_placement(vm_ctx *c, uint8_t *xcc_of_block, int n)
{
    if (!xcc_of_block || n < 1 || n > 2048) return vm_fail(VM_E_INVALID, "vm_dbg_pass_placement: bad argument");
    VM_ENTER_LOCKED(c);
    if (!c->pass_dbg.get()) { // arm: the next PASS launches record where their workgroups run
        if (int rc = c->pass_dbg.reserve(2048)) return rc;
        VM_HIP(hipMemsetAsync(c->pass_dbg.get(), 0xFF, 2048 * sizeof(uint32_t), c->stream));
        VM_HIP(hipStreamSynchronize(c->stream));
        memset(xcc_of_block, 0xFF, (size_t)n);
        return VM_OK;
    }
    std::vector<uint32_t> h(2048);
    VM_HIP(hipStreamSynchronize(c->stream));
    VM_HIP(hipMemcpy(h.data(), c->pass_dbg.get(), 2048 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; ++k) xcc_of_block[k] = (uint8_t)(h[k] & 0xFFu);
    return VM_OK;
}

extern "C" int vm_dbg_golden(vm_ctx *c, int n, const float *params, float eps, uint32_t *out)
{
    if (!params || !out || n < 1 || n > 65536) return vm_fail(VM_E_INVALID, "vm_dbg_golden: bad argument");
    if (!(eps >= 1.0f / 1024.0f && eps <= 1.0f)) return vm_fail(VM_E_INVALID, "vm_dbg_golden: eps %g (2^-10 to 1)", (double)eps);
    for (int k = 0; k < n; ++k)
        if (!(params[4 * k] >= 0.0f && params[4 * k] <= 16.0f))
            return vm_fail(VM_E_INVALID, "vm_dbg_golden: cc of case %d is %g (0 to 16)", k, (double)params[4 * k]);
    VM_ENTER_LOCKED(c);
    VmDev<float> in;
    VmDev<uint32_t> res;
    const size_t words = (size_t)n * VM_DBG_GOLDEN_WORDS;
    if (int rc = in.reserve((size_t)4 * n)) return rc;
    if (int rc = res.reserve(words)) return rc;
    hipStream_t s = c->stream;
    VM_HIP(hipMemcpyAsync(in.get(), params, (size_t)4 * n * sizeof(float), hipMemcpyHostToDevice, s));
    VM_HIP(hipMemsetAsync(res.get(), 0, words * sizeof(uint32_t), s));
    vm_launch_dbg_golden_fast(n, in.get(), eps, res.get(), s);
    VM_HIP(hipGetLastError());
    VM_HIP(hipMemcpyAsync(out, res.get(), words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_dbg_ladder(vm_ctx *c, int w, int h, const float *img0, const float *img1, int n, const float *params,
                             float eps, uint32_t *out)
{
    if (!img0 || !img1 || !params || !out || n < 1 || n > 65536 || w < 2 || h < 2 || w > 64 || h > 64)
        return vm_fail(VM_E_INVALID, "vm_dbg_ladder: bad argument");
    if (!(eps >= 1.0f / 1024.0f && eps <= 1.0f)) return vm_fail(VM_E_INVALID, "vm_dbg_ladder: eps %g (2^-10 to 1)", (double)eps);
    for (int k = 0; k < n; ++k) {
        const float *q = params + 8 * k;
        if (!(q[0] >= 0.0f && q[0] <= (float)(w - 1) && q[1] >= 0.0f && q[1] <= (float)(h - 1)))
            return vm_fail(VM_E_INVALID, "vm_dbg_ladder: pixel of case %d is (%g, %g)", k, (double)q[0], (double)q[1]);
        if (!(q[6] >= 0.0f && q[6] <= 16.0f)) return vm_fail(VM_E_INVALID, "vm_dbg_ladder: cc of case %d is %g (0 to 16)", k, (double)q[6]);
    }
    VM_ENTER_LOCKED(c);
    VmDev<float> img, in;
    VmDev<uint32_t> res;
    const size_t px = (size_t)w * h, words = (size_t)n * VM_DBG_LADDER_WORDS;
    if (int rc = img.reserve(2 * px)) return rc;
    if (int rc = in.reserve((size_t)8 * n)) return rc;
    if (int rc = res.reserve(words)) return rc;
    hipStream_t s = c->stream;
    VM_HIP(hipMemcpyAsync(img.get(), img0, px * sizeof(float), hipMemcpyHostToDevice, s));
    VM_HIP(hipMemcpyAsync(img.get() + px, img1, px * sizeof(float), hipMemcpyHostToDevice, s));
    VM_HIP(hipMemcpyAsync(in.get(), params, (size_t)8 * n * sizeof(float), hipMemcpyHostToDevice, s));
    VM_HIP(hipMemsetAsync(res.get(), 0, words * sizeof(uint32_t), s));
    vm_launch_dbg_ladder_fast(img.get(), w, h, n, in.get(), eps, res.get(), s);
    VM_HIP(hipGetLastError());
    VM_HIP(hipMemcpyAsync(out, res.get(), words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_set_tuning(vm_ctx *c, int sweep_mode, int threads, int parts)
{
    if (!c || sweep_mode < VM_SWEEP_AUTO || sweep_mode > VM_SWEEP_PASS || threads < 0 || parts < 0 ||
        (threads && (threads % 64 || threads < 256 || threads > 1024)) || parts > 64)
        return vm_fail(VM_E_INVALID, "vm_set_tuning: bad argument");
    c->sweep_mode = sweep_mode;
    c->sweep_threads = threads;
    c->sweep_parts = parts;
    return VM_OK;
}

extern "C" int vm_device_info(vm_ctx *c, char *name256, int *cus, uint64_t *hbm)
{
    VM_ENTER(c);
    hipDeviceProp_t pr;
    VM_HIP(hipGetDeviceProperties(&pr, c->device));
    if (name256) snprintf(name256, 256, "%s (%s)", pr.name, pr.gcnArchName);
    if (cus) *cus = pr.multiProcessorCount;
    if (hbm) *hbm = (uint64_t)pr.totalGlobalMem;
    return VM_OK;
}

// ---------------------------------------------------------------------------
// one slab per level: every array starts on a 256-byte boundary
int vm_level_alloc(vm_ctx *c, vm_level &l, bool with_images)
{
    size_t n = (size_t)l.rs * l.h;
    size_t off = 0;
    size_t o_v = off; off += vm_align256(n * 8);
    size_t o_img0 = off, o_img1 = off, o_luma = off, o_mean = off, o_var = off, o_tpsb = off,
           o_uib = off, o_cross = off, o_value = off, o_uiaxy = off, o_imp = off;
    if (with_images) {
        o_img0 = off; off += vm_align256(n * 4);
        o_img1 = off; off += vm_align256(n * 4);
        o_luma = off; off += vm_align256(n * 8);
        o_mean = off; off += vm_align256(n * 8);
        o_var = off; off += vm_align256(n * 8);
        o_tpsb = off; off += vm_align256(n * 8);
        o_uib = off; off += vm_align256(n * 8);
        o_cross = off; off += vm_align256(n * 4);
        o_value = off; off += vm_align256(n * 4);
        o_uiaxy = off; off += vm_align256(n * 4);
        o_imp = off; off += vm_align256((size_t)l.imp_rs * l.imp_rows * 4);
    }
    if (int rc = l.slab.reserve(off)) return rc;
    // stream-ordered: the context's stream does not synchronise with the null stream
    VM_HIP(hipMemsetAsync(l.slab.get(), 0, off, c->stream));
    char *b = l.slab.get();
    VmLevelView &V = l.view;
    V.w = l.w; V.h = l.h; V.rs = l.rs;
    V.inv_wh = 1.0f / (l.w * l.h);          // pyramid.cu:537
    V.imp_rs = l.imp_rs; V.imp_rows = l.imp_rows;
    V.v = (float2 *)(b + o_v);
    if (with_images) {
        V.img0 = (const float *)(b + o_img0); V.img1 = (const float *)(b + o_img1);
        V.luma = (float2 *)(b + o_luma); V.mean = (float2 *)(b + o_mean);
        V.var = (float2 *)(b + o_var); V.tps_b = (float2 *)(b + o_tpsb);
        V.ui_b = (float2 *)(b + o_uib); V.cross = (float *)(b + o_cross);
        V.value = (float *)(b + o_value); V.ui_axy = (float *)(b + o_uiaxy);
        V.impmask = (uint32_t *)(b + o_imp);
    } else {
        V.img0 = V.img1 = nullptr;
        V.luma = V.mean = V.var = V.tps_b = V.ui_b = nullptr;
        V.cross = V.value = V.ui_axy = nullptr;
        V.impmask = nullptr;
    }
    V.rec_a = V.rec_b = V.rec_a2 = V.rec_b2 = nullptr;
    V.rec_tag = V.rec_tag2 = nullptr;
    V.mean2 = V.var2 = V.tps_b2 = nullptr;
    V.cross2 = V.value2 = nullptr;
    V.impmask2 = nullptr;
    V.temp_ref = nullptr;
    V.temp_mask = nullptr;
    V.factor_d = 1.0f;
    V.sp_wl = V.sp_cnt = V.sp_stamp = nullptr;
    return VM_OK;
}

extern "C" int vm_pyramid_create(vm_ctx *c, int nlevels, const int *w, const int *h, vm_pyr **out)
{
    if (!c || !w || !h || !out || nlevels < 2)
        return vm_fail(VM_E_INVALID, "vm_pyramid_create: need ctx, sizes and >= 2 levels");
    for (int i = 0; i < nlevels; ++i)
        if (w[i] < 5 || h[i] < 5)
            return vm_fail(VM_E_INVALID, "vm_pyramid_create: level %d is %dx%d (min 5x5)", i, w[i], h[i]);
    VM_ON_DEVICE(c);
    vm_pyr *p = new vm_pyr();
    p->ctx = c;
    p->device = c->device;
    p->lv.resize(nlevels);
    for (int i = 0; i < nlevels; ++i) {
        vm_level &l = p->lv[i];
        l.w = w[i]; l.h = h[i];
        l.rs = (w[i] + 31) / 32 * 32;               // pyramid.cu:535
        l.imp_rs = (w[i] + 4) / 5 + 2;              // pyramid.cu:538
        l.imp_rows = (h[i] + 4) / 5 + 2;            // pyramid.cu:539
        int rc = vm_level_alloc(c, l, i != nlevels - 1);
        if (rc != VM_OK) { vm_pyramid_destroy(p); return rc; }
    }
    *out = p;
    return VM_OK;
}

extern "C" void vm_pyramid_destroy(vm_pyr *p) { vm_destroy_object(p); }

extern "C" int vm_pyramid_levels(vm_pyr *p) { return p ? (int)p->lv.size() : 0; }

static int check_level(const vm_pyr *p, int lvl, const char *fn)
{
    if (lvl < 0 || lvl >= (int)p->lv.size()) return vm_fail(VM_E_INVALID, "%s: level %d out of range", fn, lvl);
    return VM_OK;
}

int vm_pitch_resolve(const char *fn, int *pitch, size_t unit, size_t row_bytes)
{
    if (*pitch == 0) *pitch = (int)((row_bytes + unit - 1) / unit);
    if (*pitch < 0 || (size_t)*pitch * unit < row_bytes)
        return vm_fail(VM_E_INVALID, "%s: pitch %d below the row of %zu", fn, *pitch, (row_bytes + unit - 1) / unit);
    return VM_OK;
}

int vm_copy_pitched(const char *fn, hipMemcpyKind kind, void *dev, size_t dev_pitch_bytes, const void *host, int pitch,
                    size_t unit, size_t row_bytes, int h, hipStream_t s)
{
    if (int rc = vm_pitch_resolve(fn, &pitch, unit, row_bytes)) return rc;
    const size_t hp = (size_t)pitch * unit;
    if (kind == hipMemcpyHostToDevice)
        VM_HIP(hipMemcpy2DAsync(dev, dev_pitch_bytes, host, hp, row_bytes, h, kind, s));
    else
        VM_HIP(hipMemcpy2DAsync((void *)host, hp, dev, dev_pitch_bytes, row_bytes, h, kind, s));
    return VM_OK;
}

extern "C" int vm_level_dims(vm_pyr *p, int lvl, int *w, int *h, int *rs)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    if (w) *w = p->lv[lvl].w;
    if (h) *h = p->lv[lvl].h;
    if (rs) *rs = p->lv[lvl].rs;
    return VM_OK;
}

int vm_level_write_luma(vm_ctx *c, vm_level &l, const float *img0, const float *img1, int pitch, const char *fn)
{
    if (!l.view.img0) return vm_fail(VM_E_STATE, "%s: the coarsest level holds no images", fn);
    if (!img0 || !img1) return vm_fail(VM_E_INVALID, "%s: NULL image", fn);
    const float *src[2] = {img0, img1}, *dst[2] = {l.view.img0, l.view.img1};
    for (int k = 0; k < 2; ++k)
        if (int rc = vm_copy_pitched(fn, hipMemcpyHostToDevice, (void *)dst[k], l.rs * 4, src[k], pitch, 4, (size_t)l.w * 4, l.h, c->stream)) return rc;
    VM_HIP(hipStreamSynchronize(c->stream));
    return VM_OK;
}

int vm_level_copy_v(vm_ctx *c, vm_level &l, hipMemcpyKind kind, const float *v, int pitch, const char *fn)
{
    if (!v) return vm_fail(VM_E_INVALID, "%s: NULL", fn);
    if (int rc = vm_copy_pitched(fn, kind, l.view.v, l.rs * 8, v, pitch, 4, (size_t)l.w * 8, l.h, c->stream)) return rc;
    VM_HIP(hipStreamSynchronize(c->stream));
    return VM_OK;
}

extern "C" int vm_level_upload_luma(vm_pyr *p, int lvl, const float *img0, const float *img1, int pitch)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    return vm_level_write_luma(p->ctx, p->lv[lvl], img0, img1, pitch, __func__);
}

extern "C" int vm_level_set_v(vm_pyr *p, int lvl, const float *v, int pitch)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    return vm_level_copy_v(p->ctx, p->lv[lvl], hipMemcpyHostToDevice, v, pitch, __func__);
}

extern "C" int vm_level_get_v(vm_pyr *p, int lvl, float *v, int pitch)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    return vm_level_copy_v(p->ctx, p->lv[lvl], hipMemcpyDeviceToHost, v, pitch, __func__);
}

extern "C" int vm_level_get_field(vm_pyr *p, int lvl, int field, void *host)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    return vm_level_read_field(p->ctx, p->lv[lvl], field, host);
}

int vm_level_read_field(vm_ctx *c, vm_level &l, int field, void *host)
{
    if (!host) return vm_fail(VM_E_INVALID, "vm_level_get_field: NULL");
    const VmLevelView &V = l.view;
    hipStream_t s = c->stream;
    const void *src = nullptr;
    int elem = 4;
    switch (field) {
    case VM_F_IMG0: src = V.img0; break;
    case VM_F_IMG1: src = V.img1; break;
    case VM_F_V: src = V.v; elem = 8; break;
    case VM_F_LUMA: src = V.luma; elem = 8; break;
    case VM_F_MEAN: src = V.mean; elem = 8; break;
    case VM_F_VAR: src = V.var; elem = 8; break;
    case VM_F_CROSS: src = V.cross; break;
    case VM_F_VALUE: src = V.value; break;
    case VM_F_TPS_B: src = V.tps_b; elem = 8; break;
    case VM_F_UI_AXY: src = V.ui_axy; break;
    case VM_F_UI_B: src = V.ui_b; elem = 8; break;
    case VM_F_TEMP_REF: src = l.temp_ref_store; elem = 8; break;
    case VM_F_TEMP_MASK: src = l.temp_mask_store; break;
    case VM_F_COUNTER: {
        // pure function of position (morph.cu:225): not stored on the device
        float *o = (float *)host;
        for (int y = 0; y < l.h; ++y)
            for (int x = 0; x < l.w; ++x)
                o[(size_t)y * l.w + x] = (float)((std::min(y, 2) + std::min(l.h - 1 - y, 2) + 1) *
                                                  (std::min(x, 2) + std::min(l.w - 1 - x, 2) + 1));
        return VM_OK;
    }
    case VM_F_TPS_AXY: {
        // tps[B][2][2]/2 (morph.cu:242): not stored on the device
        uint32_t tab[VM_TAB_WORDS];
        build_tables(tab);
        auto cls = [](int q, int dim) { return q < 2 ? q : (q == dim - 2 ? 3 : (q == dim - 1 ? 4 : 2)); };
        float *o = (float *)host;
        for (int y = 0; y < l.h; ++y)
            for (int x = 0; x < l.w; ++x) {
                float f;
                memcpy(&f, &tab[VM_TAB_TPS + (cls(y, l.h) * 5 + cls(x, l.w)) * 25 + 12], 4);
                o[(size_t)y * l.w + x] = f / 2;
            }
        return VM_OK;
    }
    case VM_F_IMPMASK:
        if (!V.impmask) return vm_fail(VM_E_STATE, "level has no state");
        VM_HIP(hipMemcpyAsync(host, V.impmask, (size_t)l.imp_rs * l.imp_rows * 4, hipMemcpyDeviceToHost, s));
        VM_HIP(hipStreamSynchronize(s));
        return VM_OK;
    default:
        return vm_fail(VM_E_INVALID, "vm_level_get_field: unknown field %d", field);
    }
    if (!src) return vm_fail(VM_E_STATE, "vm_level_get_field: the level has no such array");
    if (int rc = vm_copy_pitched("vm_level_get_field", hipMemcpyDeviceToHost, (void *)src, (size_t)l.rs * elem, host, 0, elem, (size_t)l.w * elem, l.h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_dbg_level_set_mask(vm_pyr *p, int lvl, const uint32_t *words)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    vm_level &l = p->lv[lvl];
    if (!words) return vm_fail(VM_E_INVALID, "vm_dbg_level_set_mask: NULL");
    if (!l.has_state || !l.view.impmask) return vm_fail(VM_E_STATE, "vm_dbg_level_set_mask: level not initialised");
    hipStream_t s = p->ctx->stream;
    VM_HIP(hipMemcpyAsync(l.view.impmask, words, (size_t)l.imp_rs * l.imp_rows * 4, hipMemcpyHostToDevice, s));
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_level_clear(vm_pyr *p, int lvl)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    // Morph::clear_level frees the per-level state; the slab stays allocated
    // (288 GB of HBM: reuse beats hipFree/hipMalloc churn), it is only marked stale
    p->lv[lvl].has_state = false;
    return VM_OK;
}

// ---------------------------------------------------------------------------
static int upload_constraints(vm_ctx *c, const vm_constraint *cons, int n)
{
    if (n <= 0) return VM_OK;
    if (int rc = c->cons_dev.reserve(n)) return rc;
    VM_HIP(hipMemcpyAsync(c->cons_dev.get(), cons, (size_t)n * sizeof(vm_constraint), hipMemcpyHostToDevice, c->stream));
    VM_HIP(hipStreamSynchronize(c->stream)); // the host buffer belongs to the caller
    return VM_OK;
}

extern "C" int vm_coarse_solve(vm_pyr *p, int lvl, int w0, int h0, const vm_constraint *cons, int n)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    if (n < 0 || (n > 0 && !cons)) return vm_fail(VM_E_INVALID, "vm_coarse_solve: constraints");
    vm_level &l = p->lv[lvl];
    std::vector<float> v((size_t)2 * l.w * l.h, 0.0f);
    int rc = vm_host_coarse_solve(l.w, l.h, w0, h0, p->ctx->kp, cons, n, v.data());
    if (rc != VM_OK) return rc;
    return vm_level_set_v(p, lvl, v.data(), 0);
}

// The level kernels of one arithmetic mode, picked the way sweep_launchers() picks the sweep's.  The TEX8 modes have
// their own init_level / upsample (the reference upsamples through a linear-filtered texture too) and EXACT's splat;
// EXACT_FMA and REF_FASTMATH have no level kernels of their own and take EXACT's.
struct LevelLaunchers {
    decltype(&vm_launch_init_level_exact) init_level;
    decltype(&vm_launch_upsample_exact) upsample;
    decltype(&vm_launch_splat_exact) splat;
};
static const LevelLaunchers &level_launchers(int math_mode)
{
    static const LevelLaunchers exact = {vm_launch_init_level_exact, vm_launch_upsample_exact, vm_launch_splat_exact};
    static const LevelLaunchers fast = {vm_launch_init_level_fast, vm_launch_upsample_fast, vm_launch_splat_fast};
    static const LevelLaunchers tex8 = {vm_launch_init_level_tex8, vm_launch_upsample_tex8, vm_launch_splat_exact};
    static const LevelLaunchers tex8t = {vm_launch_init_level_tex8t, vm_launch_upsample_tex8t, vm_launch_splat_exact};
    switch (math_mode) {
    case VM_MATH_FAST: return fast;
    case VM_MATH_REF_TEX8: return tex8;
    case VM_MATH_REF_TEX8_TRUNC: return tex8t;
    default: return exact;
    }
}

// upsample(PyramidLevel&dest, PyramidLevel&orig) for one page, upsample.cu:260-286
int vm_level_upsample(vm_ctx *c, vm_level &d, const vm_level &s)
{
    level_launchers(c->math_mode).upsample(d.view.v, d.w, d.h, d.rs, s.view.v, s.w, s.h, s.rs, c->stream);
    VM_HIP(hipGetLastError());
    return VM_OK;
}

extern "C" int vm_upsample_v(vm_pyr *p, int dst, int src)
{
    VM_ENTER(p);
    if (int rc = check_level(p, dst, __func__)) return rc;
    if (int rc = check_level(p, src, __func__)) return rc;
    return vm_level_upsample(p->ctx, p->lv[dst], p->lv[src]);
}

extern "C" int vm_init_level(vm_pyr *p, int lvl, int w0, int h0, const vm_constraint *cons, int n)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    return vm_level_init(p->ctx, p->lv[lvl], w0, h0, cons, n);
}

// Morph::initialize_level for one page, morph.cu:264-390
int vm_level_init(vm_ctx *c, vm_level &l, int w0, int h0, const vm_constraint *cons, int n)
{
    if (!l.view.img0) return vm_fail(VM_E_STATE, "vm_init_level: the coarsest level is solved by vm_coarse_solve");
    if (n < 0 || (n > 0 && !cons)) return vm_fail(VM_E_INVALID, "vm_init_level: constraints");
    int rc = upload_constraints(c, cons, n);
    if (rc != VM_OK) return rc;
    const LevelLaunchers &LL = level_launchers(c->math_mode);
    LL.init_level(l.view, c->kp.ssim_clamp, c->tables.get(), c->stream);
    if (n > 0) LL.splat(l.view, w0, h0, c->cons_dev.get(), n, c->stream);
    VM_HIP(hipGetLastError());
    l.has_state = true;
    return VM_OK;
}

// Morph::optimize_level for a BATCH of frame pairs of identical geometry on one context:
// every sweep launch covers the same level of all pairs (grid.z = pair), so a level with
// too few tiles to occupy 256 CUs is filled by the batch instead -- the natural parallelism
// of the path (independent pairs).  Each pair keeps its own convergence
// flags: one that stopped improving turns into mask-pruned no-ops while the others go on.
static int optimize_level_batch(vm_pyr **ps, int n, int lvl, float max_iter, volatile const int *run_flag,
                                int fixed_work, vm_progress *out)
{
    vm_pyr *p0 = ps[0];
    vm_ctx *c = p0->ctx;
    std::vector<vm_level *> lv(n);
    for (int i = 0; i < n; ++i) {
        if (!ps[i] || ps[i]->ctx != c) return vm_fail(VM_E_INVALID, "batch: pyramids must share one context");
        if (lvl < 0 || lvl >= (int)ps[i]->lv.size()) return vm_fail(VM_E_INVALID, "batch: level %d out of range", lvl);
        lv[i] = &ps[i]->lv[lvl];
    }
    return vm_optimize_levels(c, lv.data(), n, max_iter, run_flag, fixed_work, out);
}

extern "C" int vm_optimize_level(vm_pyr *p, int lvl, float max_iter, volatile const int *run_flag,
                                 int fixed_work, vm_progress *out)
{
    VM_ENTER(p);
    if (int rc = check_level(p, lvl, __func__)) return rc;
    return optimize_level_batch(&p, 1, lvl, max_iter, run_flag, fixed_work, out);
}

extern "C" int vm_optimize_level_batch(vm_pyr **pyrs, int n, int lvl, float max_iter,
                                       volatile const int *run_flag, int fixed_work, vm_progress *out)
{
    if (!pyrs || n < 1 || !pyrs[0]) return vm_fail(VM_E_INVALID, "vm_optimize_level_batch: empty batch");
    VM_ENTER(pyrs[0]);
    return optimize_level_batch(pyrs, n, lvl, max_iter, run_flag, fixed_work, out);
}

// Morph::calculate_halfway_parametrization for a batch of pairs in lockstep; cons[i] / ncons[i] = pair i's own
// user constraints (cons == NULL: none anywhere)
extern "C" int vm_solve_batch_cons(vm_pyr **pyrs, int n, float max_iter, float drop, const vm_constraint *const *cons,
                                   const int *ncons, volatile const int *run_flag, int fixed_work, vm_progress *per_level)
{
    if (!pyrs || n < 1 || !pyrs[0]) return vm_fail(VM_E_INVALID, "vm_solve_batch: empty batch");
    if (!(drop > 0)) return vm_fail(VM_E_INVALID, "vm_solve_batch: max_iter_drop_factor must be > 0");
    if (cons && !ncons) return vm_fail(VM_E_INVALID, "vm_solve_batch_cons: constraints without their counts");
    VM_ENTER_LOCKED(pyrs[0]);
    const int L = (int)pyrs[0]->lv.size();
    const int w0 = pyrs[0]->lv[0].w, h0 = pyrs[0]->lv[0].h;
    int rc;
    for (int i = 0; i < n; ++i) {
        if (!pyrs[i] || (int)pyrs[i]->lv.size() != L) return vm_fail(VM_E_INVALID, "vm_solve_batch: pyramids must share their geometry");
        if (cons && (ncons[i] < 0 || (ncons[i] > 0 && !cons[i]))) return vm_fail(VM_E_INVALID, "vm_solve_batch_cons: constraints of pair %d", i);
        if ((rc = vm_coarse_solve(pyrs[i], L - 1, w0, h0, cons ? cons[i] : nullptr, cons ? ncons[i] : 0)) != VM_OK) return rc;
    }
    float mi = max_iter;
    std::vector<vm_progress> pr(n);
    for (int el = L - 2; el >= 0; --el) {
        if (run_flag && !*run_flag) return vm_fail(VM_E_CANCELLED, "vm_solve_batch: cancelled by run_flag");
        for (int i = 0; i < n; ++i) {
            if ((rc = vm_upsample_v(pyrs[i], el, el + 1)) != VM_OK) return rc;
            if ((rc = vm_init_level(pyrs[i], el, w0, h0, cons ? cons[i] : nullptr, cons ? ncons[i] : 0)) != VM_OK) return rc;
        }
        if ((rc = optimize_level_batch(pyrs, n, el, mi, run_flag, fixed_work, pr.data())) != VM_OK) return rc;
        if (per_level)
            for (int i = 0; i < n; ++i) per_level[(size_t)i * (L - 1) + el] = pr[i];
        mi /= drop;
    }
    return VM_OK;
}

extern "C" int vm_solve_batch(vm_pyr **pyrs, int n, float max_iter, float drop, volatile const int *run_flag,
                              int fixed_work, vm_progress *per_level)
{
    return vm_solve_batch_cons(pyrs, n, max_iter, drop, nullptr, nullptr, run_flag, fixed_work, per_level);
}

extern "C" int vm_solve(vm_pyr *p, float max_iter, float drop, const vm_constraint *cons, int n,
                        volatile const int *run_flag, int fixed_work, vm_progress *per_level)
{
    VM_ENTER_LOCKED(p);
    if (!(drop > 0)) return vm_fail(VM_E_INVALID, "vm_solve: max_iter_drop_factor must be > 0");
    const int L = (int)p->lv.size();
    const int w0 = p->lv[0].w, h0 = p->lv[0].h;
    // Morph::calculate_halfway_parametrization, morph.cu:150-168
    int rc = vm_coarse_solve(p, L - 1, w0, h0, cons, n);
    if (rc != VM_OK) return rc;
    float mi = max_iter;
    for (int el = L - 2; el >= 0; --el) {
        if (run_flag && !*run_flag) return vm_fail(VM_E_CANCELLED, "vm_solve: cancelled by run_flag");
        if ((rc = vm_upsample_v(p, el, el + 1)) != VM_OK) return rc;
        if ((rc = vm_init_level(p, el, w0, h0, cons, n)) != VM_OK) return rc;
        if ((rc = vm_optimize_level(p, el, mi, run_flag, fixed_work, per_level ? &per_level[el] : nullptr)) != VM_OK) return rc;
        // clear_level: the level's state stays allocated; v is kept for the result
        mi /= drop;
    }
    return VM_OK;
}
