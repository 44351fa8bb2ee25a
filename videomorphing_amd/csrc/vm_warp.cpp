// vm_warp.cpp -- what a frame holds for the warp kernels and what it answers about its fixed point: the layer and
// schedule uploads, and the sampling maps of the compositor's chain (render.cu:16-60, UI/RenderWidget.cpp:229-266),
// uniformly or under a transition schedule.  The render calls are vm_render_calls.cpp's.  The maps calls change nothing
// of the frame's v, path or canvases.
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
                       (uint8_t *)dev[3], 0, nullptr, nullptr, 0, 0, 0.0f, nullptr, s);
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
    f->layer_ext = false;               // the extension was the old layers': tight again until vm_frame_extend_layers
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

// the three planes of the frame's schedule: geometry, colour, and the scratch plane a call ramps its rates into
void vm_frame_schedule_planes(vm_frame *f, const float2 **geo, const float2 **color, float2 **rates)
{
    const size_t plane = (size_t)f->rs * f->h;
    *geo = f->sched.get(); *color = f->sched.get() + plane; *rates = f->sched.get() + 2 * plane;
}

extern "C" int vm_frame_transition_maps(vm_frame *f, float t, int ease, float *map0_xy, float *map1_xy, float *resid, uint8_t *flags,
                                        float *rates_gk)
{
    VM_ENTER(f);
    if (!map0_xy && !map1_xy && !resid && !flags && !rates_gk) return vm_fail(VM_E_INVALID, "%s: every output is NULL", __func__);
    if (ease != VM_EASE_LINEAR && ease != VM_EASE_SMOOTH) return vm_fail(VM_E_INVALID, "%s: ease %d", __func__, ease);
    if (!f->has_sched) return vm_fail(VM_E_STATE, "%s: the frame holds no schedule (vm_frame_upload_schedule)", __func__);
    VmTransition T{};
    T.w = f->w; T.h = f->h; T.rs = f->rs;
    T.t = t; T.ease = ease;
    T.v = f->v.get(); T.u = path_of(f);
    vm_frame_schedule_planes(f, &T.sched_geo, &T.sched_color, &T.rates);
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
