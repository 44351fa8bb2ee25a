// vm_shutter_tail.h -- what the sample loops share, for vm_shutter.hip, vm_tshutter.hip,
// vm_viewport.hip and vm_vshutter.hip: the fraction of the exposure at which sample s stands, the sum of the samples'
// colours in registers with the uniform tails' taps, and the one store of their mean; for the three shutters also the
// time of sample s and the rule by which the window form restages its window from one time to the next.
#ifndef VM_SHUTTER_TAIL_H
#define VM_SHUTTER_TAIL_H

#include "vm_chain.h"
#include "vm_layer_tap.h"
#include "vm_shutter.h"     // VM_SHUTTER_CANVAS

namespace vm_chain {

constexpr int CANVAS = VM_SHUTTER_CANVAS;
template <int C> constexpr int NACC = C == CANVAS ? 3 : C;      // accumulators per pixel

// f = ((float)s + 0.5f) / (float)N, correctly rounded
__device__ __forceinline__ float sample_fraction(int s, float n) { return __fdiv_rn((float)s + 0.5f, n); }

// t_s = open + (close - open) * f.  CLAMP: to [0, 1], where it is the chain's geo_fa (a shutter across t = 0 or 1 holds
// still outside); not where ramp clamps per texel (a shutter under a schedule)
template <bool CLAMP> __device__ __forceinline__ float sample_time(float open, float close, int s, float n)
{
    const float t = open + (close - open) * sample_fraction(s, n);
    return CLAMP ? fminf(fmaxf(t, 0.0f), 1.0f) : t;
}

// Whether time sample s stages the window at (ox, oy), for the whole workgroup, behind a barrier from the second sample on
// (every tap of the sample before has been served).  `moved`: whether the sample before left the window elsewhere.  Not
// ALWAYS (a uniform shutter): no restaging where it has not moved -- the window holds exact texels, the bits cannot
// change.  ALWAYS (under a schedule, for the rates): `moved` says whether v and u are staged with them.
template <bool ALWAYS> __device__ __forceinline__ bool restage(int s, int ox, int oy, int &at_x, int &at_y, bool &moved)
{
    ox = __builtin_amdgcn_readfirstlane(ox); oy = __builtin_amdgcn_readfirstlane(oy);
    moved = !(s && ox == at_x && oy == at_y);
    if (!ALWAYS && !moved)
        return false;
    if (s)
        __syncthreads();
    at_x = ox; at_y = oy;
    return true;
}

// A uniform value the sample loop takes from its scalar register anew in every round.  Hoisted out of the loop, what is
// derived from it -- (float)w, (float)N, 1 - color_fa, the tile's pixel, the first tap's indices and weights: some twenty
// values -- is held in vector registers across the chain and the tails, which costs the window kernels their eighth wave;
// re-derived it is a handful of instructions beside the 21 taps.
template <class T> __device__ __forceinline__ T per_sample(T v)
{
    asm volatile("" : "+s"(v));
    return v;
}

// acc += c_s: the uniform tails' taps and blend on the Landing of sample s, by the sample's colour fraction (the call's one
// color_fa, or the k the chain left under a schedule).  Args: w, h, color_from, and ext0 / ext1 / ex or layer0 / layer1 with
// their grid lw / lh and the image's place in it, lexf
template <int C, class Args> __device__ __forceinline__ void add_sample(const Args &A, const Landing &L, float color_fa, float (&acc)[NACC<C>])
{
    const float m0x = L.px - L.v.x, m0y = L.py - L.v.y;
    const float m1x = L.px + L.v.x, m1y = L.py + L.v.y;
    if constexpr (C == CANVAS) {
        const int cw = A.w + 2 * A.ex, ch = A.h + 2 * A.ex, ex = A.ex;
        float3 c;
        if (A.color_from == 0) {
            c = tap_rgb(A.ext0, cw, ch, m0x + ex + 0.5f, m0y + ex + 0.5f);
        } else if (A.color_from == 2) {
            c = tap_rgb(A.ext1, cw, ch, m1x + ex + 0.5f, m1y + ex + 0.5f);
        } else {
            const float3 c0 = tap_rgb(A.ext0, cw, ch, m0x + ex + 0.5f, m0y + ex + 0.5f);
            const float3 c1 = tap_rgb(A.ext1, cw, ch, m1x + ex + 0.5f, m1y + ex + 0.5f);
            c.x = c0.x * (1 - color_fa) + c1.x * color_fa;
            c.y = c0.y * (1 - color_fa) + c1.y * color_fa;
            c.z = c0.z * (1 - color_fa) + c1.z * color_fa;
        }
        acc[0] = acc[0] + c.x; acc[1] = acc[1] + c.y; acc[2] = acc[2] + c.z;
    } else {
        const int lw = A.lw, lh = A.lh;
        const float lexf = A.lexf;
        Texel<C> r;
        if (A.color_from == 0) {
            r = tap_layer<C>(A.layer0, lw, lh, (m0x + lexf) + 0.5f, (m0y + lexf) + 0.5f);
        } else if (A.color_from == 2) {
            r = tap_layer<C>(A.layer1, lw, lh, (m1x + lexf) + 0.5f, (m1y + lexf) + 0.5f);
        } else {
            Texel<C> c0 = tap_layer<C>(A.layer0, lw, lh, (m0x + lexf) + 0.5f, (m0y + lexf) + 0.5f);
            // 3 and 4 channels: side 1 is tapped after side 0's texels are summed (side 1's position passes through a
            // statement that stands behind the one side 0's sums pass through), or eight texels of C registers are live
            // at once: 55 / 56 registers instead of 70 / 72
            float n1x = m1x, n1y = m1y;
            if constexpr (C >= 3) {
#pragma unroll
                for (int k = 0; k < C; ++k)
                    asm volatile("" : "+v"(c0.c[k]));
                asm volatile("" : "+v"(n1x), "+v"(n1y));
            }
            const Texel<C> c1 = tap_layer<C>(A.layer1, lw, lh, (n1x + lexf) + 0.5f, (n1y + lexf) + 0.5f);
#pragma unroll
            for (int k = 0; k < C; ++k)
                r.c[k] = c0.c[k] * (1 - color_fa) + c1.c[k] * color_fa;
        }
#pragma unroll
        for (int k = 0; k < C; ++k)
            acc[k] = acc[k] + r.c[k];
    }
}

// the one store of pixel (x, y): the mean, rounded the renderer's way for the canvases.  Args: w, and rgb or out
template <int C, class Args> __device__ __forceinline__ void store_mean(const Args &A, int x, int y, const float (&acc)[NACC<C>], float n)
{
    const size_t at = (size_t)y * A.w + x;
    if constexpr (C == CANVAS) {
        uint8_t *o = A.rgb + 3 * at;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[k] = (uint8_t)((double)__fdiv_rn(acc[k], n) + 0.5);
    } else {
        Texel<C> r;
#pragma unroll
        for (int k = 0; k < C; ++k)
            r.c[k] = __fdiv_rn(acc[k], n);
        texel_store<C>(A.out, at, r);
    }
}

} // namespace vm_chain

#endif
