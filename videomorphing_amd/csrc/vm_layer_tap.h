// vm_layer_tap.h -- one bilinear tap of a tight float layer of 1..4 interleaved channels, with tap2's expression and
// clamps (vm_chain.h), for the units whose tails sample layers: vm_warp.hip and vm_shutter.hip.
#ifndef VM_LAYER_TAP_H
#define VM_LAYER_TAP_H

#include "vm_chain.h"

namespace vm_chain {

// one texel of C interleaved floats
template <int C> struct Texel { float c[C]; };

template <int C> __device__ __forceinline__ Texel<C> texel_load(const float *__restrict__ img, size_t idx)
{
    Texel<C> t;
    if constexpr (C == 2) {
        const float2 q = *(const float2 *)(img + 2 * idx);
        t.c[0] = q.x; t.c[1] = q.y;
    } else if constexpr (C == 4) {
        const float4 q = *(const float4 *)(img + 4 * idx);
        t.c[0] = q.x; t.c[1] = q.y; t.c[2] = q.z; t.c[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k)
            t.c[k] = img[(size_t)C * idx + k];
    }
    return t;
}

template <int C> __device__ __forceinline__ void texel_store(float *__restrict__ img, size_t idx, const Texel<C> &t)
{
    if constexpr (C == 2) {
        *(float2 *)(img + 2 * idx) = make_float2(t.c[0], t.c[1]);
    } else if constexpr (C == 4) {
        *(float4 *)(img + 4 * idx) = make_float4(t.c[0], t.c[1], t.c[2], t.c[3]);
    } else {
#pragma unroll
        for (int k = 0; k < C; ++k)
            img[(size_t)C * idx + k] = t.c[k];
    }
}

// tap2's bilinear expression and clamp-to-edge indices on a tight w x h layer of C channels (64-bit texel indices: a
// 4-channel layer passes 4 GiB before the field does)
template <int C> __device__ __forceinline__ Texel<C> tap_layer(const float *__restrict__ img, int w, int h, float x, float y)
{
    const Tap t = tap_at(w, h, (size_t)w, x, y);
    const float a = t.a, b = t.b;
    const Texel<C> t00 = texel_load<C>(img, t.i00), t10 = texel_load<C>(img, t.i10);
    const Texel<C> t01 = texel_load<C>(img, t.i01), t11 = texel_load<C>(img, t.i11);
    Texel<C> r;
#pragma unroll
    for (int k = 0; k < C; ++k)
        r.c[k] = (1 - a) * (1 - b) * t00.c[k] + a * (1 - b) * t10.c[k] + (1 - a) * b * t01.c[k] + a * b * t11.c[k];
    return r;
}

} // namespace vm_chain

#endif
