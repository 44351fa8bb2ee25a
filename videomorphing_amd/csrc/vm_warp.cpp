// vm_warp.cpp -- the C-ABI around vm_warp.hip: the sampling maps of the compositor's fixed point (render.cu:16-60,
// UI/RenderWidget.cpp:229-266) and float layers carried through it, uniformly or under a transition schedule.  Nothing
// here changes the frame's v, path or canvases.
#include "vm_host.h"
#include "vm_warp.h"

static const float2 *path_of(vm_frame *f) { return f->u_zero ? nullptr : f->u.get(); }

// A maps call: its N optional outputs one after the other in warp_out (256-byte aligned each; a NULL output takes no room
// and gets a NULL device pointer), launch(dev) enqueued on s, the outputs copied to the host, drained on return.
template <int N, class F> static int maps_call(vm_frame *f, void *const (&host)[N], const size_t (&bytes)[N], hipStream_t s, F launch)
{
    size_t off[N], total = 0;
    for (int k = 0; k < N; ++k) {
        off[k] = total;
        if (host[k]) total += vm_align256(bytes[k]);
    }
    if (int rc = f->warp_out.reserve(total, s)) return rc;
    void *dev[N];
    for (int k = 0; k < N; ++k) dev[k] = host[k] ? f->warp_out.get() + off[k] : nullptr;
    launch(dev);
    VM_HIP(hipGetLastError());
    for (int k = 0; k < N; ++k)
        if (host[k]) VM_HIP(hipMemcpyAsync(host[k], dev[k], bytes[k], hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_frame_sampling_maps(vm_frame *f, float geo_fa, float *map0_xy, float *map1_xy, float *resid, uint8_t *flags)
{
    VM_ENTER(f);
    if (!map0_xy && !map1_xy && !resid && !flags) return vm_fail(VM_E_INVALID, "%s: every output is NULL", __func__);
    hipStream_t s = f->ctx->stream;
    const size_t n = (size_t)f->w * f->h;
    void *const host[4] = {map0_xy, map1_xy, resid, flags};
    const size_t bytes[4] = {n * 8, n * 8, n * 4, n};
    return maps_call(f, host, bytes, s, [&](void *const *dev) {
        vm_launch_warp(f->w, f->h, f->rs, 0.0f, geo_fa, 0, f->v.get(), path_of(f), (float2 *)dev[0], (float2 *)dev[1], (float *)dev[2],
                       (uint8_t *)dev[3], 0, nullptr, nullptr, nullptr, s);
    });
}

extern "C" int vm_frame_upload_layers(vm_frame *f, int channels, const float *layer0, const float *layer1, int pitch_floats)
{
    VM_ENTER(f);
    if (channels < 1 || channels > 4) return vm_fail(VM_E_INVALID, "%s: %d channels (1..4)", __func__, channels);
    if (!layer0 || !layer1) return vm_fail(VM_E_INVALID, "%s: NULL layer", __func__);
    const size_t row = (size_t)f->w * channels * 4, one = (size_t)f->w * f->h * channels;
    if (int rc = vm_pitch_resolve(__func__, &pitch_floats, 4, row)) return rc;
    hipStream_t s = f->ctx->stream;
    const size_t off = vm_align256(one * 4) / 4;
    if (int rc = f->layers.reserve(off + one, s)) { f->layer_ch = 0; return rc; }
    f->layer_ch = 0;                    // until both copies are in
    const float *src[2] = {layer0, layer1};
    for (int k = 0; k < 2; ++k)
        if (int rc = vm_copy_pitched(__func__, hipMemcpyHostToDevice, f->layers.get() + k * off, row, src[k], pitch_floats, 4, row, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));    // the host buffers belong to the caller
    f->layer_ch = channels;
    f->layer_off = off;
    return VM_OK;
}

static int layers_dev(vm_frame *f, const char *fn, float color_fa, float geo_fa, int color_from, float *ms)
{
    if (color_from < 0 || color_from > 2) return vm_fail(VM_E_INVALID, "%s: color_from %d", fn, color_from);
    if (!f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", fn);
    vm_ctx *c = f->ctx;
    if (int rc = f->warp_out.reserve((size_t)f->w * f->h * f->layer_ch * 4, c->stream)) return rc;
    return vm_timed_launch(c, ms, [&] {
        vm_launch_warp(f->w, f->h, f->rs, color_fa, geo_fa, color_from, f->v.get(), path_of(f), nullptr, nullptr, nullptr, nullptr,
                       f->layer_ch, f->layers.get(), f->layers.get() + f->layer_off, (float *)f->warp_out.get(), c->stream);
    });
}

extern "C" int vm_render_layers_dev(vm_frame *f, float color_fa, float geo_fa, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return layers_dev(f, __func__, color_fa, geo_fa, color_from, elapsed_ms);
}

extern "C" int vm_render_layers(vm_frame *f, float color_fa, float geo_fa, int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    if (!out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    if (color_from < 0 || color_from > 2) return vm_fail(VM_E_INVALID, "%s: color_from %d", __func__, color_from);
    if (!f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", __func__);
    const size_t row = (size_t)f->w * f->layer_ch * 4;
    if (int rc = vm_pitch_resolve(__func__, &pitch_floats, 4, row)) return rc;
    if (int rc = layers_dev(f, __func__, color_fa, geo_fa, color_from, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->warp_out.get(), row, out, pitch_floats, 4, row, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

// ---------------------------------------------------------------------------
// transition control: the schedule lives in the frame, every call ramps it at its own time
extern "C" int vm_frame_upload_schedule(vm_frame *f, const float *geo_t0t1, const float *color_t0t1, int pitch_floats)
{
    VM_ENTER(f);
    if (!geo_t0t1 && !color_t0t1) return vm_fail(VM_E_INVALID, "%s: both planes are NULL", __func__);
    const size_t row = (size_t)f->w * 8, plane = (size_t)f->rs * f->h;
    if (int rc = vm_pitch_resolve(__func__, &pitch_floats, 4, row)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = f->sched.reserve(3 * plane, s)) { f->has_sched = false; return rc; }
    f->has_sched = false;               // until both planes are in
    const float *src[2] = {geo_t0t1, color_t0t1};
    std::vector<float2> uniform;        // a NULL plane: (0, 1) everywhere
    for (int k = 0; k < 2; ++k) {
        float2 *dst = f->sched.get() + k * plane;
        if (src[k]) {
            if (int rc = vm_copy_pitched(__func__, hipMemcpyHostToDevice, dst, (size_t)f->rs * 8, src[k], pitch_floats, 4, row, f->h, s)) return rc;
        } else {
            uniform.assign(plane, make_float2(0.0f, 1.0f));
            VM_HIP(hipMemcpyAsync(dst, uniform.data(), plane * 8, hipMemcpyHostToDevice, s));
        }
    }
    VM_HIP(hipStreamSynchronize(s));    // the host buffers belong to the caller
    f->has_sched = true;
    return VM_OK;
}

extern "C" int vm_frame_clear_schedule(vm_frame *f)
{
    VM_ENTER(f);
    f->has_sched = false;
    return VM_OK;
}

// what every transition call checks, and the arguments they share
static int transition_args(vm_frame *f, const char *fn, float t, int ease, int color_from, VmTransition *T)
{
    if (ease != VM_EASE_LINEAR && ease != VM_EASE_SMOOTH) return vm_fail(VM_E_INVALID, "%s: ease %d", fn, ease);
    if (color_from < 0 || color_from > 2) return vm_fail(VM_E_INVALID, "%s: color_from %d", fn, color_from);
    if (!f->has_sched) return vm_fail(VM_E_STATE, "%s: the frame holds no schedule (vm_frame_upload_schedule)", fn);
    const size_t plane = (size_t)f->rs * f->h;
    *T = VmTransition{};
    T->w = f->w; T->h = f->h; T->rs = f->rs;
    T->t = t; T->ease = ease; T->color_from = color_from;
    T->v = f->v.get(); T->u = path_of(f);
    T->sched_geo = f->sched.get(); T->sched_color = f->sched.get() + plane; T->rates = f->sched.get() + 2 * plane;
    return VM_OK;
}

// the launch of the canvas tail (layers == false) or the layer tail into warp_out, timed if ms is given
static int transition_dev(vm_frame *f, const char *fn, float t, int ease, int color_from, bool layers, float *ms)
{
    VmTransition T;
    if (int rc = transition_args(f, fn, t, ease, color_from, &T)) return rc;
    if (layers && !f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", fn);
    vm_ctx *c = f->ctx;
    if (int rc = f->warp_out.reserve((size_t)f->w * f->h * (layers ? (size_t)f->layer_ch * 4 : 3), c->stream)) return rc;
    if (layers) {
        T.channels = f->layer_ch;
        T.layer0 = f->layers.get(); T.layer1 = f->layers.get() + f->layer_off; T.out = (float *)f->warp_out.get();
    } else {
        T.channels = VM_WARP_CANVAS;
        T.ext0 = f->ext[0].get(); T.ext1 = f->ext[1].get(); T.ex = f->ex; T.rgb = (uint8_t *)f->warp_out.get();
    }
    return vm_timed_launch(c, ms, [&] { vm_launch_transition(T, c->stream); });
}

extern "C" int vm_render_transition_dev(vm_frame *f, float t, int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return transition_dev(f, __func__, t, ease, color_from, false, elapsed_ms);
}

extern "C" int vm_render_transition_layers_dev(vm_frame *f, float t, int ease, int color_from, float *elapsed_ms)
{
    VM_ENTER(f);
    return transition_dev(f, __func__, t, ease, color_from, true, elapsed_ms);
}

extern "C" int vm_render_transition(vm_frame *f, float t, int ease, int color_from, uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    if (!rgb_out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    const size_t row = (size_t)f->w * 3;
    if (int rc = vm_pitch_resolve(__func__, &pitch_bytes, 1, row)) return rc;
    if (int rc = transition_dev(f, __func__, t, ease, color_from, false, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->warp_out.get(), row, rgb_out, pitch_bytes, 1, row, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_render_transition_layers(vm_frame *f, float t, int ease, int color_from, float *out, int pitch_floats)
{
    VM_ENTER(f);
    if (!out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    // (before the pitch is judged: its row depends on the layers)
    if (!f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", __func__);
    const size_t row = (size_t)f->w * f->layer_ch * 4;
    if (int rc = vm_pitch_resolve(__func__, &pitch_floats, 4, row)) return rc;
    if (int rc = transition_dev(f, __func__, t, ease, color_from, true, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->warp_out.get(), row, out, pitch_floats, 4, row, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_frame_transition_maps(vm_frame *f, float t, int ease, float *map0_xy, float *map1_xy, float *resid, uint8_t *flags,
                                        float *rates_gk)
{
    VM_ENTER(f);
    if (!map0_xy && !map1_xy && !resid && !flags && !rates_gk) return vm_fail(VM_E_INVALID, "%s: every output is NULL", __func__);
    VmTransition T;
    if (int rc = transition_args(f, __func__, t, ease, 0, &T)) return rc;
    hipStream_t s = f->ctx->stream;
    const size_t n = (size_t)f->w * f->h;
    void *const host[5] = {map0_xy, map1_xy, resid, flags, rates_gk};
    const size_t bytes[5] = {n * 8, n * 8, n * 4, n, n * 8};
    return maps_call(f, host, bytes, s, [&](void *const *dev) {
        T.channels = 0;
        T.map0 = (float2 *)dev[0]; T.map1 = (float2 *)dev[1]; T.resid = (float *)dev[2]; T.flags = (uint8_t *)dev[3];
        T.rates_out = (float2 *)dev[4];
        vm_launch_transition(T, s);
    });
}
