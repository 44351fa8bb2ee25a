// vm_tshutter.cpp -- the C-ABI around vm_tshutter.hip: motion-blurred frames and layers under a transition schedule, the
// compositor's chain (render.cu:16-60, UI/RenderWidget.cpp:229-266) with per-texel rates integrated over a shutter in one
// launch.  Nothing here changes the frame's v, path, canvases, layers or schedule; the schedule's rate plane and
// warp_out are the call's scratch.
#include "vm_host.h"
#include "vm_tshutter.h"

// what every call checks, then the launch of the canvas tail (layers == false) or the layer tail into warp_out, timed if
// ms is given
static int tshutter_dev(vm_frame *f, const char *fn, float t_open, float t_close, int samples, float t_color, int ease,
                        int color_from, bool layers, float *ms)
{
    if (samples < 1 || samples > VM_SHUTTER_MAX_SAMPLES)
        return vm_fail(VM_E_INVALID, "%s: %d samples (1..%d)", fn, samples, (int)VM_SHUTTER_MAX_SAMPLES);
    if (ease != VM_EASE_LINEAR && ease != VM_EASE_SMOOTH) return vm_fail(VM_E_INVALID, "%s: ease %d", fn, ease);
    if (color_from < 0 || color_from > 2) return vm_fail(VM_E_INVALID, "%s: color_from %d", fn, color_from);
    if (!f->has_sched) return vm_fail(VM_E_STATE, "%s: the frame holds no schedule (vm_frame_upload_schedule)", fn);
    if (layers && !f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", fn);
    vm_ctx *c = f->ctx;
    if (int rc = f->warp_out.reserve((size_t)f->w * f->h * (layers ? (size_t)f->layer_ch * 4 : 3), c->stream)) return rc;
    const size_t plane = (size_t)f->rs * f->h;
    VmTShutter S{};
    S.w = f->w; S.h = f->h; S.rs = f->rs;
    S.t_open = t_open; S.t_close = t_close; S.t_color = t_color;
    S.samples = samples; S.ease = ease; S.color_from = color_from;
    S.vf = f->v.get(); S.uf = f->u_zero ? nullptr : f->u.get();
    S.sched_geo = f->sched.get(); S.sched_color = f->sched.get() + plane; S.rates = f->sched.get() + 2 * plane;
    if (layers) {
        S.channels = f->layer_ch;
        S.layer0 = f->layers.get(); S.layer1 = f->layers.get() + f->layer_off; S.out = (float *)f->warp_out.get();
    } else {
        S.channels = VM_SHUTTER_CANVAS;
        S.ext0 = f->ext[0].get(); S.ext1 = f->ext[1].get(); S.ex = f->ex; S.rgb = (uint8_t *)f->warp_out.get();
    }
    return vm_timed_launch(c, ms, [&] { vm_launch_tshutter(S, c->stream); });
}

extern "C" int vm_render_transition_shutter_dev(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                                int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return tshutter_dev(f, __func__, t_open, t_close, samples, t_color, ease, color_from, false, elapsed_ms);
}

extern "C" int vm_render_transition_shutter_layers_dev(vm_frame *f, float t_open, float t_close, int samples, float t_color,
                                                       int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return tshutter_dev(f, __func__, t_open, t_close, samples, t_color, ease, color_from, true, elapsed_ms);
}

extern "C" int vm_render_transition_shutter(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                            int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    if (!rgb_out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    const size_t row = (size_t)f->w * 3;
    if (int rc = vm_pitch_resolve(__func__, &pitch_bytes, 1, row)) return rc;
    if (int rc = tshutter_dev(f, __func__, t_open, t_close, samples, t_color, ease, color_from, false, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->warp_out.get(), row, rgb_out, pitch_bytes, 1, row, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_render_transition_shutter_layers(vm_frame *f, float t_open, float t_close, int samples, float t_color, int ease,
                                                   int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    if (!out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    // (before the pitch is judged: its row depends on the layers)
    if (!f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", __func__);
    const size_t row = (size_t)f->w * f->layer_ch * 4;
    if (int rc = vm_pitch_resolve(__func__, &pitch_floats, 4, row)) return rc;
    if (int rc = tshutter_dev(f, __func__, t_open, t_close, samples, t_color, ease, color_from, true, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->warp_out.get(), row, out, pitch_floats, 4, row, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}
