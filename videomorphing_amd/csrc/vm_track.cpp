// vm_track.cpp -- host side of the stage-2 point tracker (MdiEditor::AddPoint / MovePoint / Histo,
// UI/MdiEditor.cpp:1230-1393, 1516-1582): the device copies of the frames and flows of both videos,
// their flows computed as MdiEditor::OpticalFlow does (:1584-1689), the segment checks and the one
// launch of vm_track.hip per call.
#include "vm_host.h"
#include "vm_track.h"
#include "vm_flow.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

extern "C" int vm_track_create(vm_ctx *ctx, int w, int h, int depth, vm_track **out)
{
    if (!ctx || !out) return vm_fail(VM_E_INVALID, "vm_track_create: NULL argument");
    if (w < 32 || h < 32 || depth < 1 || depth > VM_TRACK_MAX_DEPTH)
        return vm_fail(VM_E_INVALID, "vm_track_create: %d frames of %d x %d (at least 32 x 32, 1..%d frames)", depth, w, h, VM_TRACK_MAX_DEPTH);
    if ((double)w * h * depth > 4e9) return vm_fail(VM_E_INVALID, "vm_track_create: %d frames of %d x %d are too large", depth, w, h);
    if (!vm_ctx_alive(ctx)) return vm_fail(VM_E_INVALID, "vm_track_create: the context was destroyed");
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    VM_ON_DEVICE(ctx);
    vm_track *t = new vm_track();
    t->ctx = ctx;
    t->device = ctx->device;
    t->w = w;
    t->h = h;
    t->depth = depth;
    const size_t n = (size_t)w * h * depth;
    for (int k = 0; k < 2; ++k) {
        int rc = t->frames[k].reserve(n);
        if (rc == VM_OK) rc = t->f[k].reserve(n);
        if (rc == VM_OK) rc = t->b[k].reserve(n);
        if (rc != VM_OK) {
            delete t;
            return rc;
        }
        t->has_frame[k].assign(depth, 0);
        t->has_f[k].assign(depth, 0);
        t->has_b[k].assign(depth, 0);
    }
    *out = t;
    return VM_OK;
}

extern "C" void vm_track_destroy(vm_track *t) { vm_destroy_object(t); }

static int check_side_frame(const vm_track *t, int side, int frame, const char *fn)
{
    if (side < 0 || side > 1) return vm_fail(VM_E_INVALID, "%s: side %d (0 or 1)", fn, side);
    if (frame < 0 || frame >= t->depth) return vm_fail(VM_E_INVALID, "%s: frame %d out of range (0..%d)", fn, frame, t->depth - 1);
    return VM_OK;
}

extern "C" int vm_track_upload_frame(vm_track *t, int side, int frame, const uint8_t *rgb, int pitch_bytes)
{
    VM_ENTER_LOCKED(t);
    if (int rc = check_side_frame(t, side, frame, __func__)) return rc;
    if (!rgb) return vm_fail(VM_E_INVALID, "vm_track_upload_frame: NULL frame");
    if (int rc = vm_pitch_resolve(__func__, &pitch_bytes, 1, (size_t)3 * t->w)) return rc;
    hipStream_t s = t->ctx->stream;
    VmDev<uint8_t> stage;
    if (int rc = stage.reserve((size_t)3 * t->w * t->h)) return rc;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyHostToDevice, stage.get(), (size_t)3 * t->w, rgb, pitch_bytes, 1, (size_t)3 * t->w, t->h, s)) return rc;
    vm_track_launch_rgba(stage.get(), 3 * t->w, t->w, t->h, t->frames[side].get() + (size_t)frame * t->w * t->h, s);
    VM_HIP(hipGetLastError());
    VM_HIP(hipStreamSynchronize(s)); // the stage is freed on return
    t->has_frame[side][frame] = 1;
    return VM_OK;
}

extern "C" int vm_track_upload_flows(vm_track *t, int side, int frame, const float *f_xy, const float *b_xy, int pitch)
{
    VM_ENTER_LOCKED(t);
    if (int rc = check_side_frame(t, side, frame, __func__)) return rc;
    if (int rc = vm_pitch_resolve(__func__, &pitch, 4, (size_t)t->w * 8)) return rc;
    for (const float *src : {f_xy, b_xy}) // every position a step can reach stays an int
        if (src)
            for (int y = 0; y < t->h; ++y)
                for (int x = 0; x < 2 * t->w; ++x) {
                    const float v = src[(size_t)y * pitch + x];
                    if (!(std::fabs(v) <= VM_TRACK_MAX_FLOW))
                        return vm_fail(VM_E_INVALID, "vm_track_upload_flows: flow value %g at (%d, %d) is not finite or beyond +-%g px",
                                       (double)v, x / 2, y, (double)VM_TRACK_MAX_FLOW);
                }
    hipStream_t s = t->ctx->stream;
    const size_t page = (size_t)t->w * t->h;
    const float *src[2] = {f_xy, b_xy};
    VmDev<float2> *dst[2] = {&t->f[side], &t->b[side]};
    for (int k = 0; k < 2; ++k)
        if (src[k])
            if (int rc = vm_copy_pitched(__func__, hipMemcpyHostToDevice, dst[k]->get() + frame * page, (size_t)t->w * 8, src[k], pitch, 4, (size_t)t->w * 8, t->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    if (f_xy) t->has_f[side][frame] = 1;
    if (b_xy) t->has_b[side][frame] = 1;
    return VM_OK;
}

extern "C" int vm_track_compute_flows(vm_track *t, const vm_flow_params *pp)
{
    VM_ENTER_LOCKED(t);
    const int w = t->w, h = t->h, d = t->depth;
    vm_flow_params p;
    if (int rc = vm_flow_resolve(pp, w, h, &p, "vm_track_compute_flows")) return rc;
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < d; ++i)
            if (!t->has_frame[k][i]) return vm_fail(VM_E_STATE, "vm_track_compute_flows: frame %d of video %d was never uploaded", i, k);
    for (int k = 0; k < 2; ++k) { // from the first write on, the flows count as supplied again only on success
        t->has_f[k].assign(d, 0);
        t->has_b[k].assign(d, 0);
    }
    hipStream_t s = t->ctx->stream;
    const size_t page = (size_t)w * h;
    for (int k = 0; k < 2; ++k) { // f[d - 1] and b[0] are zero
        VM_HIP(hipMemsetAsync(t->f[k].get() + (size_t)(d - 1) * page, 0, page * sizeof(float2), s));
        VM_HIP(hipMemsetAsync(t->b[k].get(), 0, page * sizeof(float2), s));
    }
    auto src = [&](int k, int i, float *dst) -> int {
        vm_flow_launch_grey_rgba(t->frames[k].get() + (size_t)i * page, w, h, dst, s);
        return VM_OK;
    };
    if (int rc = vm_flow_run_videos(t->ctx, w, h, d, p, src, [&](int k, int i) { return t->f[k].get() + (size_t)i * page; },
                                    [&](int k, int i) { return t->b[k].get() + (size_t)i * page; }))
        return rc;
    VM_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 2; ++k) {
        t->has_f[k].assign(d, 1);
        t->has_b[k].assign(d, 1);
    }
    return VM_OK;
}

extern "C" int vm_track_get_flows(vm_track *t, int side, int frame, float *f_xy, float *b_xy)
{
    VM_ENTER_LOCKED(t);
    if (int rc = check_side_frame(t, side, frame, __func__)) return rc;
    if ((f_xy && !t->has_f[side][frame]) || (b_xy && !t->has_b[side][frame]))
        return vm_fail(VM_E_STATE, "vm_track_get_flows: a flow of frame %d of video %d was never supplied", frame, side);
    hipStream_t s = t->ctx->stream;
    const size_t page = (size_t)t->w * t->h;
    if (f_xy) VM_HIP(hipMemcpyAsync(f_xy, t->f[side].get() + frame * page, page * 8, hipMemcpyDeviceToHost, s));
    if (b_xy) VM_HIP(hipMemcpyAsync(b_xy, t->b[side].get() + frame * page, page * 8, hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

// the frames a segment reads (its keys' and every frame it covers) and the flows it steps along
static int check_segment(const vm_track *t, const vm_track_segment &g, int i)
{
    const char *fn = "vm_track_propagate";
    const int d = t->depth;
    if (g.side < 0 || g.side > 1) return vm_fail(VM_E_INVALID, "%s: segment %d: side %d (0 or 1)", fn, i, g.side);
    if (g.frame < 0 || g.frame >= d) return vm_fail(VM_E_INVALID, "%s: segment %d: key frame %d out of range", fn, i, g.frame);
    if (std::abs(g.x) > VM_TRACK_MAX_KEY || std::abs(g.y) > VM_TRACK_MAX_KEY || (g.ofr >= 0 && (std::abs(g.ox) > VM_TRACK_MAX_KEY || std::abs(g.oy) > VM_TRACK_MAX_KEY)))
        return vm_fail(VM_E_INVALID, "%s: segment %d: a key lies beyond +-%d px", fn, i, VM_TRACK_MAX_KEY);
    int lo, hi, flo, fhi, blo, bhi; // frames [lo, hi], f[flo..fhi], b[blo..bhi]
    if (g.ofr < 0) {
        if (g.dir != 1 && g.dir != -1) return vm_fail(VM_E_INVALID, "%s: segment %d: a chain needs dir +1 or -1 (got %d)", fn, i, g.dir);
        lo = g.dir > 0 ? g.frame : 0;
        hi = g.dir > 0 ? d - 1 : g.frame;
        flo = g.dir > 0 ? g.frame : 1, fhi = g.dir > 0 ? d - 2 : 0;
        blo = 1, bhi = g.dir > 0 ? 0 : g.frame;
    } else {
        if (g.ofr >= d) return vm_fail(VM_E_INVALID, "%s: segment %d: other key frame %d out of range", fn, i, g.ofr);
        if (g.ofr == g.frame) return vm_fail(VM_E_INVALID, "%s: segment %d: both keys are on frame %d", fn, i, g.frame);
        const int sign = g.ofr > g.frame ? 1 : -1;
        if (g.dir != 0 && g.dir != sign) return vm_fail(VM_E_INVALID, "%s: segment %d: dir %d points away from the other key", fn, i, g.dir);
        lo = std::min(g.frame, g.ofr);
        hi = std::max(g.frame, g.ofr);
        flo = lo, fhi = hi - 2; // both chains stop one frame short of the far key
        blo = lo + 2, bhi = hi;
    }
    for (int s = lo; s <= hi; ++s)
        if (!t->has_frame[g.side][s]) return vm_fail(VM_E_STATE, "%s: segment %d reads frame %d of video %d, never uploaded", fn, i, s, g.side);
    for (int s = flo; s <= fhi; ++s)
        if (!t->has_f[g.side][s]) return vm_fail(VM_E_STATE, "%s: segment %d steps along f[%d] of video %d, never supplied", fn, i, s, g.side);
    for (int s = blo; s <= bhi; ++s)
        if (!t->has_b[g.side][s]) return vm_fail(VM_E_STATE, "%s: segment %d steps along b[%d] of video %d, never supplied", fn, i, s, g.side);
    return VM_OK;
}

extern "C" int vm_track_propagate(vm_track *t, const vm_track_segment *seg, int n, vm_track_point *out)
{
    VM_ENTER_LOCKED(t);
    if (n < 0 || (n > 0 && (!seg || !out))) return vm_fail(VM_E_INVALID, "vm_track_propagate: bad arguments");
    for (int i = 0; i < n; ++i)
        if (int rc = check_segment(t, seg[i], i)) return rc;
    if (n == 0) return VM_OK;
    hipStream_t s = t->ctx->stream;
    const size_t slots = (size_t)n * t->depth;
    VmDev<vm_track_segment> dseg;
    VmDev<vm_track_point> dout;
    if (int rc = dseg.reserve(n)) return rc;
    if (int rc = dout.reserve(slots)) return rc;
    std::vector<vm_track_point> host(slots);
    VM_HIP(hipMemcpyAsync(dseg.get(), seg, n * sizeof(vm_track_segment), hipMemcpyHostToDevice, s));
    vm_track_launch(dseg.get(), n, t->frames[0].get(), t->frames[1].get(), t->f[0].get(), t->f[1].get(), t->b[0].get(),
                    t->b[1].get(), t->w, t->h, t->depth, dout.get(), s);
    VM_HIP(hipGetLastError());
    VM_HIP(hipMemcpyAsync(host.data(), dout.get(), slots * sizeof(vm_track_point), hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) { // only the covered frames: the caller's other slots stay as they are
        const vm_track_segment &g = seg[i];
        int a, b;
        if (g.ofr < 0) {
            a = g.dir > 0 ? g.frame + 1 : 0;
            b = g.dir > 0 ? t->depth : g.frame;
        } else {
            a = std::min(g.frame, g.ofr) + 1;
            b = std::max(g.frame, g.ofr);
        }
        if (b > a) std::copy(host.begin() + (size_t)i * t->depth + a, host.begin() + (size_t)i * t->depth + b, out + (size_t)i * t->depth + a);
    }
    return VM_OK;
}
