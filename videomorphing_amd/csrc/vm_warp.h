// vm_warp.h -- the launcher of vm_warp.hip, called from vm_warp.cpp.
#ifndef VM_WARP_H
#define VM_WARP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// The renderer's chain with other tails.  channels == 0: the sampling maps into map0 / map1 / resid / flags (tight (h, w);
// any may be NULL); 1..4: the two tight (h, w, channels) layers through the morph into out.
void vm_launch_warp(int w, int h, int rs, float color_fa, float geo_fa, int color_from, const float2 *v, const float2 *u,
                    float2 *map0, float2 *map1, float *resid, uint8_t *flags, int channels, const float *layer0,
                    const float *layer1, float *out, hipStream_t s);

#endif
