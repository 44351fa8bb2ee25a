// vm_tshutter.h -- the launcher of vm_tshutter.hip, called from vm_render_calls.cpp.
#ifndef VM_TSHUTTER_H
#define VM_TSHUTTER_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vm_shutter.h"     // VM_SHUTTER_CANVAS, VM_SHUTTER_MAX_SAMPLES

// One shutter call under a transition schedule (vm_tshutter.hip): the chain at `samples` times between t_open
// and t_close per output pixel, each under the geometry schedule ramped at that time, the colours blended by the colour
// schedule ramped at t_color, the mean of the samples' colours.  sched_geo / sched_color: h x rs pairs (t0, t1); rates:
// the frame's scratch plane of h x rs pairs, written by the call (its .y is K).  channels 1..4: the two tight
// (h, w, channels) layers into out; VM_SHUTTER_CANVAS: RGB8 from the extended canvases into rgb (h rows of 3 w bytes).
// u may be NULL (no path).  The form of the chain is chosen by vm_render_window_form (vm_warp.h); tiles_x / ntiles are the
// launcher's.
struct VmTShutter {
    int w, h, rs;
    float t_open, t_close, t_color;
    int samples, ease, color_from;
    const float2 *vf, *uf;
    const float2 *sched_geo, *sched_color;
    float2 *rates;
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
void vm_launch_tshutter(const VmTShutter &S, hipStream_t s);

#endif
