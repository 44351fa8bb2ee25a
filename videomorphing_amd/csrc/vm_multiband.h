// vm_multiband.h -- the launcher of vm_multiband.hip, called from vm_render_calls.cpp, and the layout of the frame's
// pyramid scratch, which the launcher and vm_dbg_multiband_level share.
#ifndef VM_MULTIBAND_H
#define VM_MULTIBAND_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vmorph.h"
#include "vm_warp.h"

// Where the pyramids of one multiband call lie in the frame's scratch (floats).  Every image is PLANAR: tight planes of
// h_l x w_l floats, a level's planes `stride[l]` apart (the plane rounded up to 64 floats).  Level l holds 2 C + 1 planes
// from g[l] -- the C of G0, the C of G1, the mask -- and, for l >= 1, the C planes of R from r[l]; R of level 0 is the
// call's output (bytes, or interleaved floats) and lies in warp_out.
struct VmMbLayout {
    int levels, channels;
    int w[VM_MULTIBAND_MAX_LEVELS + 1], h[VM_MULTIBAND_MAX_LEVELS + 1];
    size_t stride[VM_MULTIBAND_MAX_LEVELS + 1], g[VM_MULTIBAND_MAX_LEVELS + 1], r[VM_MULTIBAND_MAX_LEVELS + 1];
    size_t total;
};

inline VmMbLayout vm_mb_layout(int w, int h, int channels, int levels)
{
    VmMbLayout Y{};
    Y.levels = levels; Y.channels = channels;
    size_t at = 0;
    for (int l = 0; l <= levels; ++l) {
        Y.w[l] = w; Y.h[l] = h;
        Y.stride[l] = ((size_t)w * (size_t)h + 63) & ~(size_t)63;
        Y.g[l] = at;
        at += (size_t)(2 * channels + 1) * Y.stride[l];
        Y.r[l] = at;
        if (l) at += (size_t)channels * Y.stride[l];
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    Y.total = at;
    return Y;
}

// One multiband call (vm_multiband.hip): the chain of a uniform call (rates == NULL: color_fa, geo_fa) or of a
// transition call (the schedule planes ramped at t with `ease` into rates by vm_launch_rates), the two plates and the colour
// weight written as planes into ws, reduced level by level and collapsed from the coarsest up under sharp[].  channels 1..4:
// the layers into out, interleaved floats; VM_WARP_CANVAS: RGB8 from the extended canvases into rgb.
struct VmMultiband {
    int w, h, rs;
    float color_fa, geo_fa, t;
    int ease;
    const float2 *vf, *uf;
    const float2 *sched_geo, *sched_color;
    float2 *rates;
    int channels;
    const float *layer0, *layer1;
    int lw, lh;
    float lexf;
    float *out;
    const uchar4 *ext0, *ext1;
    int ex;
    uint8_t *rgb;
    int levels;
    float sharp[VM_MULTIBAND_MAX_LEVELS + 1];
    float *ws;              // vm_mb_layout(w, h, C, levels).total floats, C = 3 for the canvases
};
void vm_launch_multiband(const VmMultiband &M, hipStream_t s);

#endif
