// vm_warp.h -- the launchers of vm_warp.hip, called from vm_warp.cpp (the maps) and vm_render_calls.cpp, and the switch
// between the chain's two forms.
#ifndef VM_WARP_H
#define VM_WARP_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vmorph.h"

// Which form of the chain (vm_chain.h) a field of pitch rs and h rows takes, for the launchers of vm_render.hip (where it is
// defined) and vm_warp.hip: the window form, unless VM_RENDER=plain asks for the plain kernels (A/B runs) or the field is
// out of the window form's reach.
bool vm_render_window_form(int rs, int h);

// The renderer's chain with other tails.  channels == 0: the sampling maps into map0 / map1 / resid / flags (tight (h, w);
// any may be NULL); 1..4: the two tight (lh, lw, channels) layers through the morph into out, the image
// at (lexf, lexf) of them: (h, w) and 0, or the extended (ch, cw) and ex (vm_frame_extend_layers).
void vm_launch_warp(int w, int h, int rs, float color_fa, float geo_fa, int color_from, const float2 *v, const float2 *u,
                    float2 *map0, float2 *map1, float *resid, uint8_t *flags, int channels, const float *layer0,
                    const float *layer1, int lw, int lh, float lexf, float *out, hipStream_t s);

// The same chain under a transition schedule (vm_warp.hip): geo_fa / color_fa are per-texel rates ramped from
// the schedule planes (h x rs pairs (t0, t1), geometry and colour) at time t with `ease`, by a pre-pass, into `rates`,
// the call's scratch plane of h x rs pairs.  channels == 0: the maps tail and rates_out (tight (h, w, 2), may be NULL); 1..4: the layers
// into out; VM_WARP_CANVAS: RGB8 from the extended canvases into rgb (h rows of 3 w bytes).
enum { VM_WARP_CANVAS = -1 };
struct VmTransition {
    int w, h, rs;
    float t;
    int ease, color_from;
    const float2 *v, *u;
    const float2 *sched_geo, *sched_color;
    float2 *rates;
    int channels;
    float2 *map0, *map1;
    float *resid;
    uint8_t *flags;
    float2 *rates_out;
    const float *layer0, *layer1;
    int lw, lh;             // the layers' grid and where the image starts in it: w, h, 0 tight; cw, ch, ex extended
    float lexf;             // (vm_frame_extend_layers)
    float *out;
    const uchar4 *ext0, *ext1;
    int ex;
    uint8_t *rgb;
};
void vm_launch_transition(const VmTransition &T, hipStream_t s);
// the pre-pass alone: T's two schedule planes ramped at T.t with T.ease into T.rates (vm_tshutter.hip takes its colour
// rates from it)
void vm_launch_rates(const VmTransition &T, hipStream_t s);

#endif
