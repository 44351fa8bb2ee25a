// vm_render_calls.cpp -- the C-ABI of the render calls, every vm_render_* of include/vmorph.h: the launchers of
// vm_render.hip, vm_warp.hip, vm_shutter.hip, vm_tshutter.hip, vm_viewport.hip, vm_vshutter.hip and vm_filter.hip (the
// compositor's chain, render.cu:16-60, UI/RenderWidget.cpp:229-266, with their tails) behind ONE host path -- check, bind, launch, download
//  -- and the carry calls of vm_carry.hip and the multiband calls of vm_multiband.hip
// on the same helpers.  Nothing here changes the frame's
// v, path, canvases, layers or schedule; the schedule's rate plane, warp_out, carry_pts and the pyramids (mb) are a call's scratch.
#include "vm_host.h"
#include "vm_warp.h"
#include "vm_shutter.h"
#include "vm_tshutter.h"
#include "vm_viewport.h"
#include "vm_vshutter.h"
#include "vm_filter.h"
#include "vm_carry.h"
#include "vm_multiband.h"
#include <vector>
#include <cmath>
#include <type_traits>

namespace {

static_assert((int)VM_WARP_CANVAS == (int)VM_SHUTTER_CANVAS, "the launchers name the canvas tail alike");
enum { VM_VIEWPORT_MAX_SIDE = 32768, VM_VIEWPORT_MAX_SAMPLES = 64 };

// What a call carries and needs (the bits of Call::what).
enum {
    VIEWPORT = 1,       // carries a vm_viewport: the output grid is the viewport's, not the frame's
    SHUTTER = 2,        // carries a sample count
    SCHEDULED = 4,      // carries an ease and needs the frame's schedule
    LAYERS = 8,         // renders the frame's layers (floats) instead of its canvases (RGB8)
    OWN_OUT = 16,       // renders into the frame's own `out` (vm_render_halfway*), not into warp_out
    FILTERED = 64,      // carries a filter (32 is the carry calls' POINTS)
    BANDS = 128         // carries a vm_bands and needs the frame's pyramid scratch
};
struct Call {
    const char *fn;     // the entry point, for the messages
    int what;
    const vm_viewport *vp;
    int samples, ease, color_from;
    int filter = VM_FILTER_BILINEAR;
    const vm_bands *bands = nullptr;
};
// ... and where its output goes: to the host (pitch in bytes for RGB8, in floats for layers; 0 = tight) and drained, or
// left on the device with the launch timed (ms may be NULL)
struct Dest {
    bool download;
    void *host;
    int pitch;
    float *ms;
};
Dest down(void *out, int pitch) { return Dest{true, out, pitch, nullptr}; }
Dest left(float *ms) { return Dest{false, nullptr, 0, ms}; }

// ---- the argument checks: VM_OK, or VM_E_INVALID with fn's message
int check_viewport(const char *fn, const vm_viewport *vp)
{
    if (!vp) return vm_fail(VM_E_INVALID, "%s: viewport is NULL", fn);
    if (!std::isfinite(vp->x0) || !std::isfinite(vp->y0))
        return vm_fail(VM_E_INVALID, "%s: viewport corner (%g, %g) is not finite", fn, (double)vp->x0, (double)vp->y0);
    if (!std::isfinite(vp->step_x) || !std::isfinite(vp->step_y) || !(vp->step_x > 0) || !(vp->step_y > 0))
        return vm_fail(VM_E_INVALID, "%s: viewport step (%g, %g) (finite, > 0)", fn, (double)vp->step_x, (double)vp->step_y);
    if (vp->out_w < 1 || vp->out_w > VM_VIEWPORT_MAX_SIDE || vp->out_h < 1 || vp->out_h > VM_VIEWPORT_MAX_SIDE)
        return vm_fail(VM_E_INVALID, "%s: output of %d x %d (1..%d each)", fn, vp->out_w, vp->out_h, (int)VM_VIEWPORT_MAX_SIDE);
    // (nx alone is bounded first: the product of two ints that passed cannot overflow)
    if (vp->nx < 1 || vp->ny < 1 || vp->nx > VM_VIEWPORT_MAX_SAMPLES || vp->ny > VM_VIEWPORT_MAX_SAMPLES ||
        vp->nx * vp->ny > VM_VIEWPORT_MAX_SAMPLES)
        return vm_fail(VM_E_INVALID, "%s: %d x %d sub-samples (each >= 1, 1..%d together)", fn, vp->nx, vp->ny,
                       (int)VM_VIEWPORT_MAX_SAMPLES);
    return VM_OK;
}

int check_samples(const char *fn, int samples)
{
    if (samples < 1 || samples > VM_SHUTTER_MAX_SAMPLES)
        return vm_fail(VM_E_INVALID, "%s: %d samples (1..%d)", fn, samples, (int)VM_SHUTTER_MAX_SAMPLES);
    return VM_OK;
}

// (after the viewport and the samples: the product of three ints that passed cannot overflow)
int check_chains(const char *fn, int samples, const vm_viewport *vp)
{
    if (samples * vp->nx * vp->ny > VM_VSHUTTER_MAX_CHAINS)
        return vm_fail(VM_E_INVALID, "%s: %d samples of %d x %d sub-samples (at most %d chains per pixel)", fn, samples, vp->nx,
                       vp->ny, (int)VM_VSHUTTER_MAX_CHAINS);
    return VM_OK;
}

int check_ease(const char *fn, int ease)
{
    if (ease != VM_EASE_LINEAR && ease != VM_EASE_SMOOTH) return vm_fail(VM_E_INVALID, "%s: ease %d", fn, ease);
    return VM_OK;
}

int check_filter(const char *fn, int filter)
{
    if (filter < VM_FILTER_BILINEAR || filter > VM_FILTER_BSPLINE) return vm_fail(VM_E_INVALID, "%s: filter %d", fn, filter);
    return VM_OK;
}

// (w x h: the frame's grid, whose coarsest level the bands must leave at least 2 x 2)
int check_bands(const char *fn, const vm_bands *b, int w, int h)
{
    if (!b) return vm_fail(VM_E_INVALID, "%s: bands is NULL", fn);
    if (b->levels < 1 || b->levels > VM_MULTIBAND_MAX_LEVELS)
        return vm_fail(VM_E_INVALID, "%s: %d levels (1..%d)", fn, b->levels, (int)VM_MULTIBAND_MAX_LEVELS);
    int cw = w, ch = h;
    for (int l = 0; l < b->levels; ++l) {
        cw = (cw + 1) / 2; ch = (ch + 1) / 2;
    }
    if (cw < 2 || ch < 2)
        return vm_fail(VM_E_INVALID, "%s: %d levels leave a coarsest level of %d x %d (at least 2 x 2)", fn, b->levels, cw, ch);
    for (int l = 0; l <= b->levels; ++l)
        if (!std::isfinite(b->sharp[l]) || !(b->sharp[l] >= 1.0f))
            return vm_fail(VM_E_INVALID, "%s: sharp[%d] = %g (finite, >= 1)", fn, l, (double)b->sharp[l]);
    return VM_OK;
}

int check_color_from(const char *fn, int color_from)
{
    if (color_from < 0 || color_from > 2) return vm_fail(VM_E_INVALID, "%s: color_from %d", fn, color_from);
    return VM_OK;
}

// the arguments a call carries, in the one order: viewport, samples, chain cap, bands, ease, filter, color_from
int check_args(const Call &k, const vm_frame *f)
{
    if (k.what & VIEWPORT)
        if (int rc = check_viewport(k.fn, k.vp)) return rc;
    if (k.what & SHUTTER)
        if (int rc = check_samples(k.fn, k.samples)) return rc;
    if ((k.what & VIEWPORT) && (k.what & SHUTTER))
        if (int rc = check_chains(k.fn, k.samples, k.vp)) return rc;
    if (k.what & BANDS)
        if (int rc = check_bands(k.fn, k.bands, f->w, f->h)) return rc;
    if (k.what & SCHEDULED)
        if (int rc = check_ease(k.fn, k.ease)) return rc;
    if (k.what & FILTERED)
        if (int rc = check_filter(k.fn, k.filter)) return rc;
    return check_color_from(k.fn, k.color_from);
}

// ---- the frame binders: a launcher's argument struct filled from the frame, field by name
const float2 *path_of(const vm_frame *f) { return f->u_zero ? nullptr : f->u.get(); }

// the field: its size and pitch, v, and the quadratic path (NULL for a zero path); VmTransition says v / u
template <class A> void bind_field(A &a, const vm_frame *f)
{
    a.w = f->w; a.h = f->h; a.rs = f->rs;
    if constexpr (std::is_same<A, VmTransition>::value) {
        a.v = f->v.get(); a.u = path_of(f);
    } else {
        a.vf = f->v.get(); a.uf = path_of(f);
    }
}

template <class A> void bind_schedule(A &a, vm_frame *f) { vm_frame_schedule_planes(f, &a.sched_geo, &a.sched_color, &a.rates); }

template <class A> void bind_viewport(A &a, const vm_viewport *vp)
{
    a.x0 = vp->x0; a.y0 = vp->y0; a.step_x = vp->step_x; a.step_y = vp->step_y;
    a.out_w = vp->out_w; a.out_h = vp->out_h; a.nx = vp->nx; a.ny = vp->ny;
}

// the tail: the frame's layers into floats at dev, or its canvases into RGB8 at dev.  The layers are the extended ones
// when the frame holds them (vm_frame_extend_layers): the canvas grid, the image at (ex, ex) -- the renderer's own + ex
template <class A> void bind_tail(A &a, const vm_frame *f, bool layers, void *dev)
{
    if (layers) {
        a.channels = f->layer_ch;
        a.out = (float *)dev;
        if (f->layer_ext) {
            a.layer0 = f->lext.get(); a.layer1 = f->lext.get() + f->lext_off;
            a.lw = f->cw; a.lh = f->ch; a.lexf = (float)f->ex;
        } else {
            a.layer0 = f->layers.get(); a.layer1 = f->layers.get() + f->layer_off;
            a.lw = f->w; a.lh = f->h; a.lexf = 0.0f;
        }
    } else {
        a.channels = VM_SHUTTER_CANVAS;
        a.ext0 = f->ext[0].get(); a.ext1 = f->ext[1].get(); a.ex = f->ex; a.rgb = (uint8_t *)dev;
    }
}

// ---- the driver: every render call after its handle guard.  NULL output (a call that downloads) -> the arguments ->
// the frame's state, "no schedule" then "no layers" -> the pitch -> the device buffer reserved, launch(dev, stream) --
// timed for a call that leaves its output there --, and for one that downloads the rows copied out and the stream drained.
template <class L> int render_call(vm_frame *f, const Call &k, const Dest &d, L launch)
{
    if (d.download && !d.host) return vm_fail(VM_E_INVALID, "%s: output is NULL", k.fn);
    if (int rc = check_args(k, f)) return rc;
    if ((k.what & SCHEDULED) && !f->has_sched)
        return vm_fail(VM_E_STATE, "%s: the frame holds no schedule (vm_frame_upload_schedule)", k.fn);
    const bool layers = (k.what & LAYERS) != 0;
    if (layers && !f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", k.fn);
    // the output grid, and one tight row of it in bytes
    const int out_w = (k.what & VIEWPORT) ? k.vp->out_w : f->w, out_h = (k.what & VIEWPORT) ? k.vp->out_h : f->h;
    const size_t unit = layers ? 4 : 1, row = (size_t)out_w * (layers ? (size_t)f->layer_ch * 4 : 3);
    int pitch = d.pitch;
    if (d.download)
        if (int rc = vm_pitch_resolve(k.fn, &pitch, unit, row)) return rc;
    vm_ctx *c = f->ctx;
    void *dev = f->out.get();
    if (!(k.what & OWN_OUT)) {
        if (int rc = f->warp_out.reserve(row * (size_t)out_h, c->stream)) return rc;
        dev = f->warp_out.get();
    }
    if (k.what & BANDS)
        if (int rc = f->mb.reserve(vm_mb_layout(f->w, f->h, layers ? f->layer_ch : 3, k.bands->levels).total, c->stream)) return rc;
    if (int rc = vm_timed_launch(c, d.ms, [&] { launch(dev, c->stream); })) return rc;
    if (!d.download) return VM_OK;
    if (int rc = vm_copy_pitched(k.fn, hipMemcpyDeviceToHost, dev, row, d.host, pitch, unit, row, out_h, c->stream)) return rc;
    VM_HIP(hipStreamSynchronize(c->stream));
    return VM_OK;
}

// ---- the families: a call's arguments into its launcher's
int halfway(vm_frame *f, const char *fn, float color_fa, float geo_fa, int color_from, const Dest &d)
{
    return render_call(f, Call{fn, OWN_OUT, nullptr, 0, 0, color_from}, d, [&](void *dev, hipStream_t s) {
        vm_launch_render((uint8_t *)dev, f->w * 3, f->w, f->h, f->rs, f->ex, color_fa, geo_fa, color_from, f->ext[0].get(),
                         f->ext[1].get(), f->v.get(), path_of(f), s);
    });
}

int layers(vm_frame *f, const char *fn, float color_fa, float geo_fa, int color_from, const Dest &d)
{
    return render_call(f, Call{fn, LAYERS, nullptr, 0, 0, color_from}, d, [&](void *dev, hipStream_t s) {
        VmTransition T{};               // (the binder's target only: the uniform launcher takes the tail field by field)
        bind_tail(T, f, true, dev);
        vm_launch_warp(f->w, f->h, f->rs, color_fa, geo_fa, color_from, f->v.get(), path_of(f), nullptr, nullptr, nullptr, nullptr,
                       T.channels, T.layer0, T.layer1, T.lw, T.lh, T.lexf, T.out, s);
    });
}

int transition(vm_frame *f, const char *fn, int tail, float t, int ease, int color_from, const Dest &d)
{
    return render_call(f, Call{fn, SCHEDULED | tail, nullptr, 0, ease, color_from}, d, [&](void *dev, hipStream_t s) {
        VmTransition T{};
        bind_field(T, f); bind_schedule(T, f); bind_tail(T, f, tail == LAYERS, dev);
        T.t = t; T.ease = ease; T.color_from = color_from;
        vm_launch_transition(T, s);
    });
}

int shutter(vm_frame *f, const char *fn, int tail, float color_fa, float geo_open, float geo_close, int samples, int color_from,
            const Dest &d)
{
    return render_call(f, Call{fn, SHUTTER | tail, nullptr, samples, 0, color_from}, d, [&](void *dev, hipStream_t s) {
        VmShutter S{};
        bind_field(S, f); bind_tail(S, f, tail == LAYERS, dev);
        S.color_fa = color_fa; S.geo_open = geo_open; S.geo_close = geo_close;
        S.samples = samples; S.color_from = color_from;
        vm_launch_shutter(S, s);
    });
}

int tshutter(vm_frame *f, const char *fn, int tail, float t_open, float t_close, int samples, float t_color, int ease,
             int color_from, const Dest &d)
{
    return render_call(f, Call{fn, SHUTTER | SCHEDULED | tail, nullptr, samples, ease, color_from}, d, [&](void *dev, hipStream_t s) {
        VmTShutter S{};
        bind_field(S, f); bind_schedule(S, f); bind_tail(S, f, tail == LAYERS, dev);
        S.t_open = t_open; S.t_close = t_close; S.t_color = t_color;
        S.samples = samples; S.ease = ease; S.color_from = color_from;
        vm_launch_tshutter(S, s);
    });
}

int viewport(vm_frame *f, const char *fn, int tail, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
             const Dest &d)
{
    return render_call(f, Call{fn, VIEWPORT | tail, vp, 0, 0, color_from}, d, [&](void *dev, hipStream_t s) {
        VmViewport V{};
        bind_field(V, f); bind_viewport(V, vp); bind_tail(V, f, tail == LAYERS, dev);
        V.color_fa = color_fa; V.geo_fa = geo_fa; V.color_from = color_from;
        vm_launch_viewport(V, s);
    });
}

// The cubic filters' coefficients (vm_filter.h): the Mitchell-Netravali family in B and C, each (float)(n / d) of doubles.
//   inner: p3 = (12 - 9B - 6C) / 6, p2 = (-18 + 12B + 6C) / 6, p0 = (6 - 2B) / 6
//   outer: q3 = (-B - 6C) / 6, q2 = (6B + 30C) / 6, q1 = (-12B - 48C) / 6, q0 = (8B + 24C) / 6
VmFiltered cubic_of(int filter)
{
    static const double T[3][7][2] = {
        {{3, 2}, {-5, 2}, {1, 1}, {-1, 2}, {5, 2}, {-4, 1}, {2, 1}},            // Catmull-Rom: B = 0, C = 1/2
        {{7, 6}, {-2, 1}, {8, 9}, {-7, 18}, {2, 1}, {-10, 3}, {16, 9}},         // Mitchell: B = 1/3, C = 1/3
        {{1, 2}, {-1, 1}, {2, 3}, {-1, 6}, {1, 1}, {-2, 1}, {4, 3}},            // B-spline: B = 1, C = 0
    };
    const double (&t)[7][2] = T[filter - VM_FILTER_CATMULL_ROM];
    VmFiltered F{};
    F.p3 = (float)(t[0][0] / t[0][1]); F.p2 = (float)(t[1][0] / t[1][1]); F.p0 = (float)(t[2][0] / t[2][1]);
    F.q3 = (float)(t[3][0] / t[3][1]); F.q2 = (float)(t[4][0] / t[4][1]); F.q1 = (float)(t[5][0] / t[5][1]);
    F.q0 = (float)(t[6][0] / t[6][1]);
    return F;
}

// a viewport call with a filter on its last taps (vm_filter.hip).  VM_FILTER_BILINEAR is the viewport call
// itself: the same launcher, hence the same bits
int filtered(vm_frame *f, const char *fn, int tail, const vm_viewport *vp, int filter, float color_fa, float geo_fa, int color_from,
             const Dest &d)
{
    return render_call(f, Call{fn, VIEWPORT | FILTERED | tail, vp, 0, 0, color_from, filter}, d, [&](void *dev, hipStream_t s) {
        if (filter == VM_FILTER_BILINEAR) {
            VmViewport V{};
            bind_field(V, f); bind_viewport(V, vp); bind_tail(V, f, tail == LAYERS, dev);
            V.color_fa = color_fa; V.geo_fa = geo_fa; V.color_from = color_from;
            vm_launch_viewport(V, s);
            return;
        }
        VmFiltered V = cubic_of(filter);
        bind_field(V, f); bind_viewport(V, vp); bind_tail(V, f, tail == LAYERS, dev);
        V.color_fa = color_fa; V.geo_fa = geo_fa; V.color_from = color_from;
        vm_launch_filtered(V, s);
    });
}

// the uniform family (sched == 0: t_open / t_close are geo_open / geo_close, the schedule planes stay NULL, t_color and
// ease are not read) or the scheduled one (sched == SCHEDULED: color_fa is not read)
int vshutter(vm_frame *f, const char *fn, int sched, int tail, const vm_viewport *vp, float color_fa, float t_open, float t_close,
             int samples, float t_color, int ease, int color_from, const Dest &d)
{
    return render_call(f, Call{fn, VIEWPORT | SHUTTER | sched | tail, vp, samples, ease, color_from}, d, [&](void *dev, hipStream_t s) {
        VmVShutter S{};
        bind_field(S, f); bind_viewport(S, vp); bind_tail(S, f, tail == LAYERS, dev);
        if (sched) bind_schedule(S, f);
        S.color_fa = color_fa; S.t_open = t_open; S.t_close = t_close; S.t_color = t_color;
        S.samples = samples; S.ease = ease; S.color_from = color_from;
        vm_launch_vshutter(S, s);
    });
}

// a uniform (sched == 0: t and ease are not read) or a transition call (sched == SCHEDULED: color_fa and geo_fa are not
// read) blended band by band (vm_multiband.hip); the calls are the blend: color_from is 1
int multiband(vm_frame *f, const char *fn, int sched, int tail, const vm_bands *bands, float color_fa, float geo_fa, float t, int ease,
              const Dest &d)
{
    Call k{fn, BANDS | sched | tail, nullptr, 0, ease, 1};
    k.bands = bands;
    const int rc = render_call(f, k, d, [&](void *dev, hipStream_t s) {
        VmMultiband M{};
        bind_field(M, f); bind_tail(M, f, tail == LAYERS, dev);
        if (sched) bind_schedule(M, f);
        M.color_fa = color_fa; M.geo_fa = geo_fa; M.t = t; M.ease = ease;
        M.levels = bands->levels;
        for (int l = 0; l <= bands->levels; ++l) M.sharp[l] = bands->sharp[l];
        M.ws = f->mb.get();
        vm_launch_multiband(M, s);
        // (what vm_dbg_multiband_level reads: set once the launches are enqueued)
        f->mb_levels = bands->levels; f->mb_channels = tail == LAYERS ? f->layer_ch : 3; f->mb_layers = tail == LAYERS;
    });
    return rc;
}

// ---- the carry calls (vm_carry.hip): the same path -- check, bind, launch, download -- with up to six
// optional outputs in the place of one pitched image.  `what`: POINTS (pts / n are the start points; without it the start
// points are the frame's pixel grid) and SCHEDULED.  host: out, halfway, pos0, pos1, resid, flags.  A call that leaves its
// output on the device (the dense _dev twins) writes what the dense call can give -- out, resid, flags -- and downloads
// nothing.  NULL outputs and arrays -> the arguments (n, nt, the times, ease) -> the frame's state -> the outputs one after
// the other in warp_out (256-byte aligned each), the points uploaded into carry_pts, the launch, the copies out, drained.
enum { POINTS = 32 };

int carry(vm_frame *f, const char *fn, int what, const float *pts, int n, float from, int ease, const float *to, int nt,
          void *const (&host)[6], const Dest &d)
{
    const bool points = (what & POINTS) != 0;
    bool want[6];
    bool any = false;
    for (int k = 0; k < 6; ++k) {
        want[k] = d.download ? host[k] != nullptr : (k == 0 || k >= 4);
        any = any || want[k];
    }
    if (!any) return vm_fail(VM_E_INVALID, "%s: every output is NULL", fn);
    if (points && !pts) return vm_fail(VM_E_INVALID, "%s: the points are NULL", fn);
    if (!to) return vm_fail(VM_E_INVALID, "%s: the to-times are NULL", fn);
    if (points && (n < 1 || n > VM_CARRY_MAX_POINTS))
        return vm_fail(VM_E_INVALID, "%s: %d points (1..%d)", fn, n, (int)VM_CARRY_MAX_POINTS);
    const int max_nt = points ? VM_CARRY_MAX_TIMES : VM_CARRY_MAX_DENSE_TIMES;
    if (nt < 1 || nt > max_nt) return vm_fail(VM_E_INVALID, "%s: %d to-times (1..%d)", fn, nt, max_nt);
    if (!std::isfinite(from)) return vm_fail(VM_E_INVALID, "%s: the from-time %g is not finite", fn, (double)from);
    for (int k = 0; k < nt; ++k)
        if (!std::isfinite(to[k])) return vm_fail(VM_E_INVALID, "%s: to-time %d, %g, is not finite", fn, k, (double)to[k]);
    if (what & SCHEDULED)
        if (int rc = check_ease(fn, ease)) return rc;
    if ((what & SCHEDULED) && !f->has_sched)
        return vm_fail(VM_E_STATE, "%s: the frame holds no schedule (vm_frame_upload_schedule)", fn);
    vm_ctx *c = f->ctx;
    hipStream_t s = c->stream;
    const size_t N = points ? (size_t)n : (size_t)f->w * f->h;
    const size_t bytes[6] = {(size_t)nt * N * 8, N * 8, N * 8, N * 8, N * 4, N};
    size_t off[6], total = 0;
    for (int k = 0; k < 6; ++k) {
        off[k] = total;
        if (want[k]) total += vm_align256(bytes[k]);
    }
    if (int rc = f->warp_out.reserve(total, s)) return rc;
    if (points)
        if (int rc = f->carry_pts.reserve(N, s)) return rc;
    void *dev[6];
    for (int k = 0; k < 6; ++k) dev[k] = want[k] ? f->warp_out.get() + off[k] : nullptr;
    VmCarry C{};
    bind_field(C, f);
    if (what & SCHEDULED) bind_schedule(C, f);
    C.from = from; C.ease = ease;
    C.pts = f->carry_pts.get(); C.n = n;
    C.out = (float2 *)dev[0]; C.halfway = (float2 *)dev[1]; C.pos0 = (float2 *)dev[2]; C.pos1 = (float2 *)dev[3];
    C.resid = (float *)dev[4]; C.flags = (uint8_t *)dev[5];
    C.nt = nt;
    for (int k = 0; k < nt; ++k) C.to[k] = to[k];
    if (points) VM_HIP(hipMemcpyAsync(f->carry_pts.get(), pts, N * 8, hipMemcpyHostToDevice, s));
    if (int rc = vm_timed_launch(c, d.ms, [&] { points ? vm_launch_carry_points(C, s) : vm_launch_motion_maps(C, s); })) return rc;
    if (!d.download) return VM_OK;
    for (int k = 0; k < 6; ++k)
        if (host[k]) VM_HIP(hipMemcpyAsync(host[k], dev[k], bytes[k], hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));    // the host buffers belong to the caller
    return VM_OK;
}

// the points call downloads and may be timed too; the dense calls do one or the other
Dest down_timed(float *ms) { return Dest{true, nullptr, 0, ms}; }

} // namespace

// ---- the entry points: the handle guard under the call's own name, then its family
extern "C" int vm_render_halfway(vm_frame *f, float color_fa, float geo_fa, int color_from, uint8_t *rgb, int pitch)
{
    VM_ENTER(f);
    return halfway(f, __func__, color_fa, geo_fa, color_from, down(rgb, pitch));
}

extern "C" int vm_render_halfway_dev(vm_frame *f, float color_fa, float geo_fa, int color_from, float *ms)
{
    VM_ENTER(f);
    return halfway(f, __func__, color_fa, geo_fa, color_from, left(ms));
}

extern "C" int vm_render_layers(vm_frame *f, float color_fa, float geo_fa, int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    return layers(f, __func__, color_fa, geo_fa, color_from, down(out, pitch_floats));
}

extern "C" int vm_render_layers_dev(vm_frame *f, float color_fa, float geo_fa, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return layers(f, __func__, color_fa, geo_fa, color_from, left(elapsed_ms));
}

extern "C" int vm_render_transition(vm_frame *f, float t, int ease, int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return transition(f, __func__, 0, t, ease, color_from, down(rgb_out, pitch_bytes));
}

extern "C" int vm_render_transition_dev(vm_frame *f, float t, int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return transition(f, __func__, 0, t, ease, color_from, left(elapsed_ms));
}

extern "C" int vm_render_transition_layers(vm_frame *f, float t, int ease, int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    return transition(f, __func__, LAYERS, t, ease, color_from, down(out, pitch_floats));
}

extern "C" int vm_render_transition_layers_dev(vm_frame *f, float t, int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return transition(f, __func__, LAYERS, t, ease, color_from, left(elapsed_ms));
}

extern "C" int vm_render_shutter(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples, int color_from,
                                 uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return shutter(f, __func__, 0, color_fa, geo_open, geo_close, samples, color_from, down(rgb_out, pitch_bytes));
}

extern "C" int vm_render_shutter_dev(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples, int color_from,
                                     float *elapsed_ms)
{
    VM_ENTER(f);
    return shutter(f, __func__, 0, color_fa, geo_open, geo_close, samples, color_from, left(elapsed_ms));
}

extern "C" int vm_render_shutter_layers(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples, int color_from,
                                        float *out, int pitch_floats)
{
    VM_ENTER(f);
    return shutter(f, __func__, LAYERS, color_fa, geo_open, geo_close, samples, color_from, down(out, pitch_floats));
}

extern "C" int vm_render_shutter_layers_dev(vm_frame *f, float color_fa, float geo_open, float geo_close, int samples,
                                            int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return shutter(f, __func__, LAYERS, color_fa, geo_open, geo_close, samples, color_from, left(elapsed_ms));
}

extern "C" int vm_render_transition_shutter(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                            int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return tshutter(f, __func__, 0, t_open, t_close, samples, t_color, ease, color_from, down(rgb_out, pitch_bytes));
}

extern "C" int vm_render_transition_shutter_dev(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                                int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return tshutter(f, __func__, 0, t_open, t_close, samples, t_color, ease, color_from, left(elapsed_ms));
}

extern "C" int vm_render_transition_shutter_layers(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                                   int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    return tshutter(f, __func__, LAYERS, t_open, t_close, samples, t_color, ease, color_from, down(out, pitch_floats));
}

extern "C" int vm_render_transition_shutter_layers_dev(vm_frame *f, float t_open, float t_close, int samples, float t_color,
                                                       int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return tshutter(f, __func__, LAYERS, t_open, t_close, samples, t_color, ease, color_from, left(elapsed_ms));
}

extern "C" int vm_render_viewport(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                  uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return viewport(f, __func__, 0, vp, color_fa, geo_fa, color_from, down(rgb_out, pitch_bytes));
}

extern "C" int vm_render_viewport_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                      float *elapsed_ms)
{
    VM_ENTER(f);
    return viewport(f, __func__, 0, vp, color_fa, geo_fa, color_from, left(elapsed_ms));
}

extern "C" int vm_render_viewport_layers(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                         float *out, int pitch_floats)
{
    VM_ENTER(f);
    return viewport(f, __func__, LAYERS, vp, color_fa, geo_fa, color_from, down(out, pitch_floats));
}

extern "C" int vm_render_viewport_layers_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                             float *elapsed_ms)
{
    VM_ENTER(f);
    return viewport(f, __func__, LAYERS, vp, color_fa, geo_fa, color_from, left(elapsed_ms));
}

extern "C" int vm_frame_render_viewport_filtered(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                                 int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return filtered(f, __func__, 0, vp, filter, color_fa, geo_fa, color_from, down(rgb_out, pitch_bytes));
}

extern "C" int vm_frame_render_viewport_filtered_dev(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                                     int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return filtered(f, __func__, 0, vp, filter, color_fa, geo_fa, color_from, left(elapsed_ms));
}

extern "C" int vm_frame_render_viewport_filtered_layers(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                                        int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    return filtered(f, __func__, LAYERS, vp, filter, color_fa, geo_fa, color_from, down(out, pitch_floats));
}

extern "C" int vm_frame_render_viewport_filtered_layers_dev(vm_frame *f, const vm_viewport *vp, int filter, float color_fa, float geo_fa,
                                                            int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return filtered(f, __func__, LAYERS, vp, filter, color_fa, geo_fa, color_from, left(elapsed_ms));
}

extern "C" int vm_render_viewport_shutter(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close,
                                          int samples, int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return vshutter(f, __func__, 0, 0, vp, color_fa, geo_open, geo_close, samples, 0.0f, VM_EASE_LINEAR, color_from,
                    down(rgb_out, pitch_bytes));
}

extern "C" int vm_render_viewport_shutter_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close,
                                              int samples, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter(f, __func__, 0, 0, vp, color_fa, geo_open, geo_close, samples, 0.0f, VM_EASE_LINEAR, color_from, left(elapsed_ms));
}

extern "C" int vm_render_viewport_shutter_layers(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open,
                                                 float geo_close, int samples, int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    return vshutter(f, __func__, 0, LAYERS, vp, color_fa, geo_open, geo_close, samples, 0.0f, VM_EASE_LINEAR, color_from,
                    down(out, pitch_floats));
}

extern "C" int vm_render_viewport_shutter_layers_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open,
                                                     float geo_close, int samples, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter(f, __func__, 0, LAYERS, vp, color_fa, geo_open, geo_close, samples, 0.0f, VM_EASE_LINEAR, color_from,
                    left(elapsed_ms));
}

extern "C" int vm_render_viewport_transition_shutter(vm_frame *f, const vm_viewport *vp, float t_open, float t_close, int samples,
                                                     float t_color, int ease, int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return vshutter(f, __func__, SCHEDULED, 0, vp, 0.0f, t_open, t_close, samples, t_color, ease, color_from, down(rgb_out, pitch_bytes));
}

extern "C" int vm_render_viewport_transition_shutter_dev(vm_frame *f, const vm_viewport *vp, float t_open, float t_close,
                                                         int samples, float t_color, int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter(f, __func__, SCHEDULED, 0, vp, 0.0f, t_open, t_close, samples, t_color, ease, color_from, left(elapsed_ms));
}

extern "C" int vm_render_viewport_transition_shutter_layers(vm_frame *f, const vm_viewport *vp, float t_open, float t_close,
                                                            int samples, float t_color, int ease, int color_from, float *out,
                                                            int pitch_floats)
{
    VM_ENTER(f);
    return vshutter(f, __func__, SCHEDULED, LAYERS, vp, 0.0f, t_open, t_close, samples, t_color, ease, color_from,
                    down(out, pitch_floats));
}

extern "C" int vm_render_viewport_transition_shutter_layers_dev(vm_frame *f, const vm_viewport *vp, float t_open, float t_close,
                                                                int samples, float t_color, int ease, int color_from,
                                                                float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter(f, __func__, SCHEDULED, LAYERS, vp, 0.0f, t_open, t_close, samples, t_color, ease, color_from, left(elapsed_ms));
}

// ---- points and motion vectors through the morph (vm_carry.hip)
extern "C" int vm_frame_carry_points(vm_frame *f, float from_fa, const float *pts_xy, int n, const float *to_fa, int nt,
                                     float *out_xy, float *halfway_xy, float *pos0_xy, float *pos1_xy, float *resid,
                                     uint8_t *flags, float *elapsed_ms)
{
    VM_ENTER(f);
    void *const host[6] = {out_xy, halfway_xy, pos0_xy, pos1_xy, resid, flags};
    return carry(f, __func__, POINTS, pts_xy, n, from_fa, VM_EASE_LINEAR, to_fa, nt, host, down_timed(elapsed_ms));
}

extern "C" int vm_frame_carry_points_transition(vm_frame *f, float t_from, int ease, const float *pts_xy, int n,
                                                const float *t_to, int nt, float *out_xy, float *halfway_xy, float *pos0_xy,
                                                float *pos1_xy, float *resid, uint8_t *flags, float *elapsed_ms)
{
    VM_ENTER(f);
    void *const host[6] = {out_xy, halfway_xy, pos0_xy, pos1_xy, resid, flags};
    return carry(f, __func__, POINTS | SCHEDULED, pts_xy, n, t_from, ease, t_to, nt, host, down_timed(elapsed_ms));
}

extern "C" int vm_frame_motion_maps(vm_frame *f, float from_fa, const float *to_fa, int nt, float *out_xy, float *resid,
                                    uint8_t *flags)
{
    VM_ENTER(f);
    void *const host[6] = {out_xy, nullptr, nullptr, nullptr, resid, flags};
    return carry(f, __func__, 0, nullptr, 0, from_fa, VM_EASE_LINEAR, to_fa, nt, host, down_timed(nullptr));
}

extern "C" int vm_frame_motion_maps_dev(vm_frame *f, float from_fa, const float *to_fa, int nt, float *elapsed_ms)
{
    VM_ENTER(f);
    void *const host[6] = {};
    return carry(f, __func__, 0, nullptr, 0, from_fa, VM_EASE_LINEAR, to_fa, nt, host, left(elapsed_ms));
}

extern "C" int vm_frame_transition_motion_maps(vm_frame *f, float t_from, int ease, const float *t_to, int nt, float *out_xy,
                                               float *resid, uint8_t *flags)
{
    VM_ENTER(f);
    void *const host[6] = {out_xy, nullptr, nullptr, nullptr, resid, flags};
    return carry(f, __func__, SCHEDULED, nullptr, 0, t_from, ease, t_to, nt, host, down_timed(nullptr));
}

extern "C" int vm_frame_transition_motion_maps_dev(vm_frame *f, float t_from, int ease, const float *t_to, int nt,
                                                   float *elapsed_ms)
{
    VM_ENTER(f);
    void *const host[6] = {};
    return carry(f, __func__, SCHEDULED, nullptr, 0, t_from, ease, t_to, nt, host, left(elapsed_ms));
}

// ---- the two plates blended band by band (vm_multiband.hip)
extern "C" int vm_frame_render_multiband(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa, uint8_t *rgb_out,
                                         int pitch_bytes)
{
    VM_ENTER(f);
    return multiband(f, __func__, 0, 0, bands, color_fa, geo_fa, 0.0f, VM_EASE_LINEAR, down(rgb_out, pitch_bytes));
}

extern "C" int vm_frame_render_multiband_dev(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa, float *elapsed_ms)
{
    VM_ENTER(f);
    return multiband(f, __func__, 0, 0, bands, color_fa, geo_fa, 0.0f, VM_EASE_LINEAR, left(elapsed_ms));
}

extern "C" int vm_frame_render_multiband_layers(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa, float *out,
                                                int pitch_floats)
{
    VM_ENTER(f);
    return multiband(f, __func__, 0, LAYERS, bands, color_fa, geo_fa, 0.0f, VM_EASE_LINEAR, down(out, pitch_floats));
}

extern "C" int vm_frame_render_multiband_layers_dev(vm_frame *f, const vm_bands *bands, float color_fa, float geo_fa,
                                                    float *elapsed_ms)
{
    VM_ENTER(f);
    return multiband(f, __func__, 0, LAYERS, bands, color_fa, geo_fa, 0.0f, VM_EASE_LINEAR, left(elapsed_ms));
}

extern "C" int vm_frame_render_multiband_transition(vm_frame *f, const vm_bands *bands, float t, int ease, uint8_t *rgb_out,
                                                    int pitch_bytes)
{
    VM_ENTER(f);
    return multiband(f, __func__, SCHEDULED, 0, bands, 0.0f, 0.0f, t, ease, down(rgb_out, pitch_bytes));
}

extern "C" int vm_frame_render_multiband_transition_dev(vm_frame *f, const vm_bands *bands, float t, int ease, float *elapsed_ms)
{
    VM_ENTER(f);
    return multiband(f, __func__, SCHEDULED, 0, bands, 0.0f, 0.0f, t, ease, left(elapsed_ms));
}

extern "C" int vm_frame_render_multiband_transition_layers(vm_frame *f, const vm_bands *bands, float t, int ease, float *out,
                                                           int pitch_floats)
{
    VM_ENTER(f);
    return multiband(f, __func__, SCHEDULED, LAYERS, bands, 0.0f, 0.0f, t, ease, down(out, pitch_floats));
}

extern "C" int vm_frame_render_multiband_transition_layers_dev(vm_frame *f, const vm_bands *bands, float t, int ease,
                                                               float *elapsed_ms)
{
    VM_ENTER(f);
    return multiband(f, __func__, SCHEDULED, LAYERS, bands, 0.0f, 0.0f, t, ease, left(elapsed_ms));
}

// one level of what the last multiband call left: the planes gathered into tight (h_l, w_l, C) floats on the host
extern "C" int vm_dbg_multiband_level(vm_frame *f, int what, int level, float *out)
{
    VM_ENTER(f);
    if (!out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    if (what < VM_MB_G0 || what > VM_MB_OUT) return vm_fail(VM_E_INVALID, "%s: what %d", __func__, what);
    if (!f->mb_levels) return vm_fail(VM_E_STATE, "%s: the frame has made no multiband call", __func__);
    if (level < 0 || level > f->mb_levels) return vm_fail(VM_E_INVALID, "%s: level %d (0..%d)", __func__, level, f->mb_levels);
    if (what == VM_MB_OUT && level == 0 && !f->mb_layers)
        return vm_fail(VM_E_INVALID, "%s: level 0 of an RGB8 call is the call's bytes", __func__);
    hipStream_t s = f->ctx->stream;
    const int C = f->mb_channels;
    const VmMbLayout Y = vm_mb_layout(f->w, f->h, C, f->mb_levels);
    const size_t n = (size_t)Y.w[level] * Y.h[level];
    if (what == VM_MB_OUT && level == 0) {      // the layer call's output, interleaved already
        VM_HIP(hipMemcpyAsync(out, f->warp_out.get(), n * C * sizeof(float), hipMemcpyDeviceToHost, s));
        VM_HIP(hipStreamSynchronize(s));
        return VM_OK;
    }
    const int planes = what == VM_MB_MASK ? 1 : C;
    const float *src = f->mb.get() + (what == VM_MB_OUT ? Y.r[level] : Y.g[level] + (what == VM_MB_G1 ? C : what == VM_MB_MASK ? 2 * C : 0) * Y.stride[level]);
    std::vector<float> host(n * planes);
    for (int c = 0; c < planes; ++c)
        VM_HIP(hipMemcpyAsync(host.data() + c * n, src + c * Y.stride[level], n * sizeof(float), hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    for (int c = 0; c < planes; ++c)
        for (size_t i = 0; i < n; ++i) out[i * planes + c] = host[c * n + i];
    return VM_OK;
}
