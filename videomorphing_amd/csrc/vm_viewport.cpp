// vm_viewport.cpp -- the C-ABI around vm_viewport.hip: any viewport of the morph at any size, supersampled, the
// compositor's chain (render.cu:16-60, UI/RenderWidget.cpp:229-266) from the sub-sample points of an output grid in one
// launch.  Nothing here changes the frame's v, path, canvases, layers or schedule.
#include "vm_host.h"
#include "vm_viewport.h"
#include <cmath>

enum { VM_VIEWPORT_MAX_SIDE = 32768, VM_VIEWPORT_MAX_SAMPLES = 64 };

// what every viewport call checks of its viewport and colour source (vm_host.h: vm_vshutter.cpp checks the same)
int vm_viewport_check(const char *fn, const vm_viewport *vp, int color_from)
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
    if (color_from < 0 || color_from > 2) return vm_fail(VM_E_INVALID, "%s: color_from %d", fn, color_from);
    return VM_OK;
}

// bytes of one tight output row
static size_t viewport_row(const vm_frame *f, const vm_viewport *vp, bool layers)
{
    return (size_t)vp->out_w * (layers ? (size_t)f->layer_ch * 4 : 3);
}

// the launch of the canvas tail (layers == false) or the layer tail into warp_out, reserved by the output's size, timed if
// ms is given; the viewport has been checked
static int viewport_dev(vm_frame *f, const char *fn, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                        bool layers, float *ms)
{
    if (layers && !f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", fn);
    vm_ctx *c = f->ctx;
    if (int rc = f->warp_out.reserve(viewport_row(f, vp, layers) * (size_t)vp->out_h, c->stream)) return rc;
    VmViewport V{};
    V.w = f->w; V.h = f->h; V.rs = f->rs;
    V.color_fa = color_fa; V.geo_fa = geo_fa; V.color_from = color_from;
    V.x0 = vp->x0; V.y0 = vp->y0; V.step_x = vp->step_x; V.step_y = vp->step_y;
    V.out_w = vp->out_w; V.out_h = vp->out_h; V.nx = vp->nx; V.ny = vp->ny;
    V.vf = f->v.get(); V.uf = f->u_zero ? nullptr : f->u.get();
    if (layers) {
        V.channels = f->layer_ch;
        V.layer0 = f->layers.get(); V.layer1 = f->layers.get() + f->layer_off; V.out = (float *)f->warp_out.get();
    } else {
        V.channels = VM_SHUTTER_CANVAS;
        V.ext0 = f->ext[0].get(); V.ext1 = f->ext[1].get(); V.ex = f->ex; V.rgb = (uint8_t *)f->warp_out.get();
    }
    return vm_timed_launch(c, ms, [&] { vm_launch_viewport(V, c->stream); });
}

extern "C" int vm_render_viewport_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                      float *elapsed_ms)
{
    VM_ENTER(f);
    if (int rc = vm_viewport_check(__func__, vp, color_from)) return rc;
    return viewport_dev(f, __func__, vp, color_fa, geo_fa, color_from, false, elapsed_ms);
}

extern "C" int vm_render_viewport_layers_dev(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                             float *elapsed_ms)
{
    VM_ENTER(f);
    if (int rc = vm_viewport_check(__func__, vp, color_from)) return rc;
    return viewport_dev(f, __func__, vp, color_fa, geo_fa, color_from, true, elapsed_ms);
}

extern "C" int vm_render_viewport(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                  uint8_t *rgb_out, int pitch_bytes)
{
    VM_ENTER(f);
    if (!rgb_out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    if (int rc = vm_viewport_check(__func__, vp, color_from)) return rc;
    const size_t row = viewport_row(f, vp, false);
    if (int rc = vm_pitch_resolve(__func__, &pitch_bytes, 1, row)) return rc;
    if (int rc = viewport_dev(f, __func__, vp, color_fa, geo_fa, color_from, false, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->warp_out.get(), row, rgb_out, pitch_bytes, 1, row, vp->out_h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_render_viewport_layers(vm_frame *f, const vm_viewport *vp, float color_fa, float geo_fa, int color_from,
                                         float *out, int pitch_floats)
{
    VM_ENTER(f);
    if (!out) return vm_fail(VM_E_INVALID, "%s: output is NULL", __func__);
    if (int rc = vm_viewport_check(__func__, vp, color_from)) return rc;
    // (before the pitch is judged: its row depends on the layers)
    if (!f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", __func__);
    const size_t row = viewport_row(f, vp, true);
    if (int rc = vm_pitch_resolve(__func__, &pitch_floats, 4, row)) return rc;
    if (int rc = viewport_dev(f, __func__, vp, color_fa, geo_fa, color_from, true, nullptr)) return rc;
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->warp_out.get(), row, out, pitch_floats, 4, row, vp->out_h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}
