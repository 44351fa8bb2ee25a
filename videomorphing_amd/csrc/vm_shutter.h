// vm_shutter.h -- the launcher of vm_shutter.hip, called from vm_render_calls.cpp.
#ifndef VM_SHUTTER_H
#define VM_SHUTTER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// One shutter call (vm_shutter.hip): the chain at `samples` times between geo_open and geo_close per output
// pixel, the mean of the samples' colours.  channels 1..4: the two tight (h, w, channels) layers into out;
// VM_SHUTTER_CANVAS: RGB8 from the extended canvases into rgb (h rows of 3 w bytes).  u may be NULL (no path).  The form of
// the chain is chosen by vm_render_window_form (vm_warp.h); tiles_x / ntiles are the launcher's.
enum { VM_SHUTTER_CANVAS = -1, VM_SHUTTER_MAX_SAMPLES = 64 };
struct VmShutter {
    int w, h, rs;
    float color_fa, geo_open, geo_close;
    int samples, color_from;
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
void vm_launch_shutter(const VmShutter &S, hipStream_t s);

#endif
