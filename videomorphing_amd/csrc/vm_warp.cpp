// vm_warp.cpp -- the C-ABI around vm_warp.hip: the sampling maps of the compositor's fixed point (render.cu:16-60,
// UI/RenderWidget.cpp:229-266) and float layers carried through it.  Nothing here changes the frame's v, path or canvases.
#include "vm_host.h"
#include "vm_warp.h"

static const float2 *path_of(vm_frame *f) { return f->u_zero ? nullptr : f->u.get(); }

extern "C" int vm_frame_sampling_maps(vm_frame *f, float geo_fa, float *map0_xy, float *map1_xy, float *resid, uint8_t *flags)
{
    VM_ENTER(f);
    if (!map0_xy && !map1_xy && !resid && !flags) return vm_fail(VM_E_INVALID, "%s: every output is NULL", __func__);
    hipStream_t s = f->ctx->stream;
    // the outputs asked for, one after the other in the staging buffer (256-byte aligned each)
    const size_t n = (size_t)f->w * f->h;
    void *host[4] = {map0_xy, map1_xy, resid, flags};
    const size_t bytes[4] = {n * 8, n * 8, n * 4, n};
    size_t off[4], total = 0;
    for (int k = 0; k < 4; ++k) {
        off[k] = total;
        if (host[k]) total += vm_align256(bytes[k]);
    }
    if (int rc = f->warp_out.reserve(total, s)) return rc;
    char *d = f->warp_out.get();
    vm_launch_warp(f->w, f->h, f->rs, 0.0f, geo_fa, 0, f->v.get(), path_of(f), map0_xy ? (float2 *)(d + off[0]) : nullptr,
                   map1_xy ? (float2 *)(d + off[1]) : nullptr, resid ? (float *)(d + off[2]) : nullptr,
                   flags ? (uint8_t *)(d + off[3]) : nullptr, 0, nullptr, nullptr, nullptr, s);
    VM_HIP(hipGetLastError());
    for (int k = 0; k < 4; ++k)
        if (host[k]) VM_HIP(hipMemcpyAsync(host[k], d + off[k], bytes[k], hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
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
    if (ms) VM_HIP(hipEventRecord(c->ev0.get(), c->stream));
    vm_launch_warp(f->w, f->h, f->rs, color_fa, geo_fa, color_from, f->v.get(), path_of(f), nullptr, nullptr, nullptr, nullptr,
                   f->layer_ch, f->layers.get(), f->layers.get() + f->layer_off, (float *)f->warp_out.get(), c->stream);
    VM_HIP(hipGetLastError());
    if (ms) {
        VM_HIP(hipEventRecord(c->ev1.get(), c->stream));
        VM_HIP(hipEventSynchronize(c->ev1.get()));
        VM_HIP(hipEventElapsedTime(ms, c->ev0.get(), c->ev1.get()));
    }
    return VM_OK;
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
