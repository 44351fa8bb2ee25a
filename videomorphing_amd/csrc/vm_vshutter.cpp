// vm_vshutter.cpp -- the C-ABI around vm_vshutter.hip: any viewport of the morph over a shutter, uniformly and under a
// transition schedule, the compositor's chain (render.cu:16-60, UI/RenderWidget.cpp:229-266) from the sub-sample points of
// an output grid at the sample times of a shutter in one launch.  Nothing here changes the frame's v, path, canvases,
// layers or schedule; the schedule's rate plane and warp_out are the call's scratch.
#include "vm_host.h"
#include "vm_vshutter.h"

namespace {

// one call's arguments: the uniform family (scheduled == false: color_fa, t_open / t_close are geo_open / geo_close) or
// the scheduled one (t_color, ease)
struct Call {
    const vm_viewport *vp;
    bool scheduled;
    float color_fa, t_open, t_close, t_color;
    int samples, ease, color_from;
};

// what every call checks of its arguments before it looks at the frame
int vshutter_check(const char *fn, const Call &k)
{
    if (int rc = vm_viewport_check(fn, k.vp, k.color_from)) return rc;
    if (k.samples < 1 || k.samples > VM_SHUTTER_MAX_SAMPLES)
        return vm_fail(VM_E_INVALID, "%s: %d samples (1..%d)", fn, k.samples, (int)VM_SHUTTER_MAX_SAMPLES);
    if (k.samples * k.vp->nx * k.vp->ny > VM_VSHUTTER_MAX_CHAINS)
        return vm_fail(VM_E_INVALID, "%s: %d samples of %d x %d sub-samples (at most %d chains per pixel)", fn, k.samples,
                       k.vp->nx, k.vp->ny, (int)VM_VSHUTTER_MAX_CHAINS);
    if (k.scheduled && k.ease != VM_EASE_LINEAR && k.ease != VM_EASE_SMOOTH) return vm_fail(VM_E_INVALID, "%s: ease %d", fn, k.ease);
    return VM_OK;
}

// bytes of one tight output row
size_t vshutter_row(const vm_frame *f, const vm_viewport *vp, bool layers)
{
    return (size_t)vp->out_w * (layers ? (size_t)f->layer_ch * 4 : 3);
}

// the launch of the canvas tail (layers == false) or the layer tail into warp_out, reserved by the output's size, timed if
// ms is given; the arguments have been checked
int vshutter_dev(vm_frame *f, const char *fn, const Call &k, bool layers, float *ms)
{
    if (k.scheduled && !f->has_sched) return vm_fail(VM_E_STATE, "%s: the frame holds no schedule (vm_frame_upload_schedule)", fn);
    if (layers && !f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", fn);
    vm_ctx *c = f->ctx;
    const vm_viewport *vp = k.vp;
    if (int rc = f->warp_out.reserve(vshutter_row(f, vp, layers) * (size_t)vp->out_h, c->stream)) return rc;
    VmVShutter S{};
    S.w = f->w; S.h = f->h; S.rs = f->rs;
    S.color_fa = k.color_fa; S.t_open = k.t_open; S.t_close = k.t_close; S.t_color = k.t_color;
    S.samples = k.samples; S.ease = k.ease; S.color_from = k.color_from;
    S.x0 = vp->x0; S.y0 = vp->y0; S.step_x = vp->step_x; S.step_y = vp->step_y;
    S.out_w = vp->out_w; S.out_h = vp->out_h; S.nx = vp->nx; S.ny = vp->ny;
    S.vf = f->v.get(); S.uf = f->u_zero ? nullptr : f->u.get();
    if (k.scheduled) {
        const size_t plane = (size_t)f->rs * f->h;
        S.sched_geo = f->sched.get(); S.sched_color = f->sched.get() + plane; S.rates = f->sched.get() + 2 * plane;
    }
    if (layers) {
        S.channels = f->layer_ch;
        S.layer0 = f->layers.get(); S.layer1 = f->layers.get() + f->layer_off; S.out = (float *)f->warp_out.get();
    } else {
        S.channels = VM_SHUTTER_CANVAS;
        S.ext0 = f->ext[0].get(); S.ext1 = f->ext[1].get(); S.ex = f->ex; S.rgb = (uint8_t *)f->warp_out.get();
    }
    return vm_timed_launch(c, ms, [&] { vm_launch_vshutter(S, c->stream); });
}

// a _dev call: checked, launched, the output left in warp_out
int vshutter_left(vm_frame *f, const char *fn, const Call &k, bool layers, float *ms)
{
    if (int rc = vshutter_check(fn, k)) return rc;
    return vshutter_dev(f, fn, k, layers, ms);
}

// a call that downloads: out of `unit`-byte elements (RGB8 bytes: 1, layer floats: 4), pitch in elements
int vshutter_down(vm_frame *f, const char *fn, const Call &k, bool layers, void *out, int pitch)
{
    if (!out) return vm_fail(VM_E_INVALID, "%s: output is NULL", fn);
    if (int rc = vshutter_check(fn, k)) return rc;
    // (before the pitch is judged: its row depends on the layers)
    if (layers && !f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", fn);
    const size_t unit = layers ? 4 : 1, row = vshutter_row(f, k.vp, layers);
    if (int rc = vm_pitch_resolve(fn, &pitch, unit, row)) return rc;
    if (int rc = vshutter_dev(f, fn, k, layers, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(fn, hipMemcpyDeviceToHost, f->warp_out.get(), row, out, pitch, unit, row, k.vp->out_h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

Call uniform(const vm_viewport *vp, float color_fa, float geo_open, float geo_close, int samples, int color_from)
{
    return Call{vp, false, color_fa, geo_open, geo_close, 0.0f, samples, VM_EASE_LINEAR, color_from};
}

Call scheduled(const vm_viewport *vp, float t_open, float t_close, int samples, float t_color, int ease, int color_from)
{
    return Call{vp, true, 0.0f, t_open, t_close, t_color, samples, ease, color_from};
}

} // namespace

extern "C" int vm_render_viewport_shutter(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close,
                                          int samples, int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return vshutter_down(f, __func__, uniform(vp, color_fa, geo_open, geo_close, samples, color_from), false, rgb_out, pitch_bytes);
}

extern "C" int vm_render_viewport_shutter_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open, float geo_close,
                                              int samples, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter_left(f, __func__, uniform(vp, color_fa, geo_open, geo_close, samples, color_from), false, elapsed_ms);
}

extern "C" int vm_render_viewport_shutter_layers(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open,
                                                 float geo_close, int samples, int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    return vshutter_down(f, __func__, uniform(vp, color_fa, geo_open, geo_close, samples, color_from), true, out, pitch_floats);
}

extern "C" int vm_render_viewport_shutter_layers_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_open,
                                                     float geo_close, int samples, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter_left(f, __func__, uniform(vp, color_fa, geo_open, geo_close, samples, color_from), true, elapsed_ms);
}

extern "C" int vm_render_viewport_transition_shutter(vm_frame *f, const vm_viewport *vp, float t_open, float t_close, int samples,
                                                     float t_color, int ease, int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    return vshutter_down(f, __func__, scheduled(vp, t_open, t_close, samples, t_color, ease, color_from), false, rgb_out, pitch_bytes);
}

extern "C" int vm_render_viewport_transition_shutter_dev(vm_frame *f, const vm_viewport *vp, float t_open, float t_close,
                                                         int samples, float t_color, int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter_left(f, __func__, scheduled(vp, t_open, t_close, samples, t_color, ease, color_from), false, elapsed_ms);
}

extern "C" int vm_render_viewport_transition_shutter_layers(vm_frame *f, const vm_viewport *vp, float t_open, float t_close,
                                                            int samples, float t_color, int ease, int color_from, float *out,
                                                            int pitch_floats)
{
    VM_ENTER(f);
    return vshutter_down(f, __func__, scheduled(vp, t_open, t_close, samples, t_color, ease, color_from), true, out, pitch_floats);
}

extern "C" int vm_render_viewport_transition_shutter_layers_dev(vm_frame *f, const vm_viewport *vp, float t_open, float t_close,
                                                                int samples, float t_color, int ease, int color_from,
                                                                float *elapsed_ms)
{
    VM_ENTER(f);
    return vshutter_left(f, __func__, scheduled(vp, t_open, t_close, samples, t_color, ease, color_from), true, elapsed_ms);
}
