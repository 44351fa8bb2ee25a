// vm_error.cpp -- C-ABI of the error view (include/vmorph.h, "error view"): the energy totals of a
// level, one plane of per-pixel terms, and the heat-ramp image of a plane, for a frame pair's level and for a page of a
// video level.  The reference only has the menu entry (UI/MdiEditor.cpp:1928-1933); the terms are those of
// Algorithm/morph.cu:730-761.  Kernels: vm_error.hip.  Every call is stream-ordered on the owning context's stream,
// drained on return, and reads the level without changing it.
#include "vm_host.h"
#include "vm_error.h"

#include <cstring>
#include <vector>

namespace {

const int kMaxBatch = 4096, kMaxSide = 16384;

int check_what(int what, const char *fn)
{
    if (what < VM_ERR_SSIM || what > VM_ERR_ALL)
        return vm_fail(VM_E_INVALID, "%s: what %d (0 ssim, 1 tps, 2 ui, 3 temp, 4 all)", fn, what);
    return VM_OK;
}

int pyr_level(vm_pyr *p, int lvl, const char *fn, vm_level **out)
{
    if (lvl < 0 || lvl >= (int)p->lv.size()) return vm_fail(VM_E_INVALID, "%s: level %d out of range", fn, lvl);
    *out = &p->lv[lvl];
    return VM_OK;
}

int video_page(vm_video *v, int lvl, int page, const char *fn, vm_level **out)
{
    if (lvl < 0 || lvl >= (int)v->pages.size()) return vm_fail(VM_E_INVALID, "%s: level %d out of range", fn, lvl);
    if (page < 0 || page >= v->depth[lvl])
        return vm_fail(VM_E_INVALID, "%s: page %d out of range (level %d has %d)", fn, page, lvl, v->depth[lvl]);
    *out = &v->pages[lvl][page].lv;
    return VM_OK;
}

// the level as the kernels read it; a level without initialised state is refused
int job_of(const vm_level &l, const char *fn, VmErrJob *J)
{
    const VmLevelView &V = l.view;
    if (!V.value) return vm_fail(VM_E_STATE, "%s: the coarsest level holds only v", fn);
    if (!l.has_state) return vm_fail(VM_E_STATE, "%s: the level holds no initialised state (before vm_init_level, or after vm_level_clear)", fn);
    *J = VmErrJob{};
    J->value = V.value; J->ui_axy = V.ui_axy; J->v = V.v; J->tps_b = V.tps_b; J->ui_b = V.ui_b;
    J->temp_ref = V.temp_mask ? V.temp_ref : nullptr; // flag == true <=> the view carries the temporal arrays
    J->temp_mask = V.temp_mask;
    J->factor_d = V.factor_d;
    return VM_OK;
}

// k_error_terms over n levels of one geometry: totals to out5n (n x 5), plane `what` of level 0 to `plane` (n == 1)
int run_terms(vm_ctx *c, vm_level *const *lv, int n, double *out5n, int what, float *plane, int pitch, const char *fn)
{
    const vm_level &l0 = *lv[0];
    hipStream_t s = c->stream;
    const int nblk = vm_error_blocks(l0.w, l0.h);
    const size_t jobs_b = vm_align256((size_t)n * sizeof(VmErrJob)), part_b = vm_align256((size_t)n * nblk * 5 * sizeof(double)),
                 tot_b = (size_t)n * 5 * sizeof(double), tk_words = (size_t)n * vm_error_ticket_words(nblk);
    if (plane)
        if (int rc = vm_pitch_resolve(fn, &pitch, 4, (size_t)l0.w * 4)) return rc;
    if (int rc = c->err_ws.reserve(jobs_b + part_b + tot_b, s)) return rc;
    if (int rc = c->err_tickets.reserve(tk_words, s)) return rc;
    if (int rc = c->err_host.reserve(jobs_b + tot_b, s)) return rc;
    if (plane)
        if (int rc = c->err_out.reserve((size_t)l0.rs * l0.h * 4, s)) return rc;
    VmErrJob *hj = (VmErrJob *)c->err_host.get();
    for (int i = 0; i < n; ++i) {
        if (int rc = job_of(*lv[i], fn, &hj[i])) return rc;
        if (plane) hj[i].plane[what] = (float *)c->err_out.get();
    }
    char *ws = c->err_ws.get();
    double *part = (double *)(ws + jobs_b), *totals = (double *)(ws + jobs_b + part_b);
    VM_HIP(hipMemcpyAsync(ws, hj, (size_t)n * sizeof(VmErrJob), hipMemcpyHostToDevice, s));
    VM_HIP(hipMemsetAsync(c->err_tickets.get(), 0, tk_words * sizeof(unsigned), s)); // every call starts from zeroed counters
    vm_launch_error_terms((const VmErrJob *)ws, n, l0.w, l0.h, l0.rs, l0.view.inv_wh, c->kp, part, c->err_tickets.get(), totals, s);
    VM_HIP(hipGetLastError());
    double *ht = (double *)(c->err_host.get() + jobs_b);
    VM_HIP(hipMemcpyAsync(ht, totals, tot_b, hipMemcpyDeviceToHost, s));
    if (plane)
        if (int rc = vm_copy_pitched(fn, hipMemcpyDeviceToHost, c->err_out.get(), (size_t)l0.rs * 4, plane, pitch, 4, (size_t)l0.w * 4, l0.h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    if (out5n) memcpy(out5n, ht, tot_b);
    return VM_OK;
}

int run_image(vm_ctx *c, vm_level &l, int what, float gain, int w0, int h0, uint8_t *rgb, int pitch, const char *fn)
{
    if (int rc = check_what(what, fn)) return rc;
    if (w0 < 1 || h0 < 1 || w0 > kMaxSide || h0 > kMaxSide) return vm_fail(VM_E_INVALID, "%s: image of %dx%d (1 .. %d a side)", fn, w0, h0, kMaxSide);
    if (!rgb) return vm_fail(VM_E_INVALID, "%s: rgb is NULL", fn);
    if (int rc = vm_pitch_resolve(fn, &pitch, 1, (size_t)w0 * 3)) return rc;
    VmErrJob J;
    if (int rc = job_of(l, fn, &J)) return rc;
    hipStream_t s = c->stream;
    if (int rc = c->err_out.reserve((size_t)w0 * 3 * h0, s)) return rc;
    uint8_t *dev = (uint8_t *)c->err_out.get();
    vm_launch_error_image(J, l.w, l.h, l.rs, l.view.inv_wh, c->kp, what, gain, w0, h0, dev, w0 * 3, s);
    VM_HIP(hipGetLastError());
    if (int rc = vm_copy_pitched(fn, hipMemcpyDeviceToHost, dev, (size_t)w0 * 3, rgb, pitch, 1, (size_t)w0 * 3, h0, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

int run_map(vm_ctx *c, vm_level *l, int what, float *plane, int pitch, const char *fn)
{
    if (int rc = check_what(what, fn)) return rc;
    if (!plane) return vm_fail(VM_E_INVALID, "%s: plane is NULL", fn);
    return run_terms(c, &l, 1, nullptr, what, plane, pitch, fn);
}

} // namespace

extern "C" int vm_level_energy(vm_pyr *p, int lvl, double *out5)
{
    VM_ENTER_LOCKED(p);
    vm_level *l;
    if (int rc = pyr_level(p, lvl, __func__, &l)) return rc;
    if (!out5) return vm_fail(VM_E_INVALID, "vm_level_energy: out5 is NULL");
    return run_terms(p->ctx, &l, 1, out5, 0, nullptr, 0, __func__);
}

extern "C" int vm_level_energy_batch(vm_pyr **pyrs, int n, int lvl, double *out5n)
{
    if (!pyrs || n < 1 || !pyrs[0]) return vm_fail(VM_E_INVALID, "vm_level_energy_batch: empty batch");
    VM_ENTER_LOCKED(pyrs[0]);
    if (n > kMaxBatch) return vm_fail(VM_E_INVALID, "vm_level_energy_batch: %d pairs (at most %d)", n, kMaxBatch);
    if (!out5n) return vm_fail(VM_E_INVALID, "vm_level_energy_batch: out5n is NULL");
    vm_ctx *c = pyrs[0]->ctx;
    std::vector<vm_level *> lv(n);
    for (int i = 0; i < n; ++i) {
        if (!pyrs[i] || pyrs[i]->ctx != c) return vm_fail(VM_E_INVALID, "vm_level_energy_batch: pyramids must share one context");
        if (int rc = pyr_level(pyrs[i], lvl, __func__, &lv[i])) return rc;
        if (lv[i]->w != lv[0]->w || lv[i]->h != lv[0]->h) return vm_fail(VM_E_INVALID, "vm_level_energy_batch: pyramids must share their geometry");
    }
    return run_terms(c, lv.data(), n, out5n, 0, nullptr, 0, __func__);
}

extern "C" int vm_level_error_map(vm_pyr *p, int lvl, int what, float *plane, int pitch)
{
    VM_ENTER_LOCKED(p);
    vm_level *l;
    if (int rc = pyr_level(p, lvl, __func__, &l)) return rc;
    return run_map(p->ctx, l, what, plane, pitch, __func__);
}

extern "C" int vm_level_error_image(vm_pyr *p, int lvl, int what, float gain, int w0, int h0, uint8_t *rgb, int pitch_bytes)
{
    VM_ENTER_LOCKED(p);
    vm_level *l;
    if (int rc = pyr_level(p, lvl, __func__, &l)) return rc;
    return run_image(p->ctx, *l, what, gain, w0, h0, rgb, pitch_bytes, __func__);
}

extern "C" int vm_video_energy(vm_video *v, int lvl, int page, double *out5)
{
    VM_ENTER_LOCKED(v);
    vm_level *l;
    if (int rc = video_page(v, lvl, page, __func__, &l)) return rc;
    if (!out5) return vm_fail(VM_E_INVALID, "vm_video_energy: out5 is NULL");
    return run_terms(v->ctx, &l, 1, out5, 0, nullptr, 0, __func__);
}

extern "C" int vm_video_error_map(vm_video *v, int lvl, int page, int what, float *plane, int pitch)
{
    VM_ENTER_LOCKED(v);
    vm_level *l;
    if (int rc = video_page(v, lvl, page, __func__, &l)) return rc;
    return run_map(v->ctx, l, what, plane, pitch, __func__);
}

extern "C" int vm_video_error_image(vm_video *v, int lvl, int page, int what, float gain, int w0, int h0, uint8_t *rgb,
                                    int pitch_bytes)
{
    VM_ENTER_LOCKED(v);
    vm_level *l;
    if (int rc = video_page(v, lvl, page, __func__, &l)) return rc;
    return run_image(v->ctx, *l, what, gain, w0, h0, rgb, pitch_bytes, __func__);
}
