// vm_vshutter.h -- the launcher of vm_vshutter.hip, called from vm_render_calls.cpp.
#ifndef VM_VSHUTTER_H
#define VM_VSHUTTER_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vm_shutter.h"     // VM_SHUTTER_CANVAS, VM_SHUTTER_MAX_SAMPLES

// samples * nx * ny of one call, at most: a 4 x 4 grid at 16 times.  A condition of the interface (include/vmorph.h), not
// a measurement.
enum { VM_VSHUTTER_MAX_CHAINS = 256 };

// One viewport call over a shutter (vm_vshutter.hip): the chain from the nx x ny sub-sample points of every
// pixel of an out_w x out_h grid laid over the halfway domain (vm_viewport.h) at `samples` times between t_open and t_close
// (vm_shutter.h, vm_tshutter.h), the mean of the samples' colours.  sched_geo == NULL, the uniform family: the times are
// clamped to [0, 1] and are the chain's geo_fa, the colours are blended by color_fa; ease, t_color, sched_color and rates are
// not read.  Otherwise the scheduled family: the geometry schedule is ramped at every time, the colour schedule once at
// t_color, by the call's pre-pass, into rates (the frame's scratch plane of h x rs pairs; its .y is K); color_fa is not
// read.  w, h, rs: the field.  channels 1..4: the two tight (h, w, channels) layers into out, tight (out_h, out_w,
// channels); VM_SHUTTER_CANVAS: RGB8 from the extended canvases into rgb (out_h rows of 3 out_w bytes).  u may be NULL (no
// path).  The form of the chain is chosen by vm_render_window_form (vm_warp.h) and the steps (the window form takes steps
// up to 1); tiles_x / ntiles are the launcher's.
struct VmVShutter {
    int w, h, rs;
    float color_fa;
    float t_open, t_close, t_color;
    int samples, ease, color_from;
    float x0, y0, step_x, step_y;
    int out_w, out_h, nx, ny;
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
void vm_launch_vshutter(const VmVShutter &S, hipStream_t s);

#endif
