// vm_viewport.h -- the launcher of vm_viewport.hip, called from vm_render_calls.cpp.
#ifndef VM_VIEWPORT_H
#define VM_VIEWPORT_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vm_shutter.h"     // VM_SHUTTER_CANVAS

// One viewport call (vm_viewport.hip): the chain from the nx x ny sub-sample points of every pixel of an
// out_w x out_h grid laid over the halfway domain at (x0, y0) with (step_x, step_y) field pixels per output pixel, the mean
// of the samples' colours.  w, h, rs: the field.  channels 1..4: the two tight (h, w, channels) layers into out, tight
// (out_h, out_w, channels); VM_SHUTTER_CANVAS: RGB8 from the extended canvases into rgb (out_h rows of 3 out_w bytes).  u may
// be NULL (no path).  The form of the chain is chosen by vm_render_window_form (vm_warp.h) and the steps (the window form
// takes steps up to 1); tiles_x / ntiles are the launcher's.
struct VmViewport {
    int w, h, rs;
    float color_fa, geo_fa;
    int color_from;
    float x0, y0, step_x, step_y;
    int out_w, out_h, nx, ny;
    const float2 *vf, *uf;
    int channels;
    const float *layer0, *layer1;
    int lw, lh;             // the layers' grid and where the image starts in it: w, h, 0 tight; cw, ch, ex extended
    float lexf;             // (vm_frame_extend_layers)
    float *out;
    const uchar4 *ext0, *ext1;
    int ex;
    uint8_t *rgb;
    int tiles_x, ntiles;
};
void vm_launch_viewport(const VmViewport &V, hipStream_t s);

#endif
