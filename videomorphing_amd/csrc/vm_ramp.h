// vm_ramp.h -- the ramp of a transition schedule, for the units that turn a schedule into rates: vm_warp.hip
// ramps both planes once per call, in a pre-pass (k_rates); vm_tshutter.hip ramps the geometry plane at every sample
// time of a shutter while it reads it, through a Ramped in the place of the chain's rate plane; vm_carry.hip
// ramps the four geometry texels of one landing point at every to-time, through a GeoTap.
#ifndef VM_RAMP_H
#define VM_RAMP_H

#include "vm_chain.h"
#include "../../include/vmorph.h"

namespace vm_chain {

// the ramp of one texel's schedule (t0, t1) at time t
__device__ __forceinline__ float ramp(float2 s, float t, int ease)
{
    const float d = s.y - s.x;
    const float r = d > 0.0f ? fminf(fmaxf(__fdiv_rn(t - s.x, d), 0.0f), 1.0f) : (t >= s.x ? 1.0f : 0.0f);
    return ease == VM_EASE_SMOOTH ? (r * r) * (3.0f - 2.0f * r) : r;
}

// A rate plane that is never stored: G is the geometry schedule ramped at t where it is read, K the .y of a plane k_rates
// has ramped at the call's colour time (all of the field's pitch).  The chain reads its rates through rate_at (the window
// form: staging, the centre, a tap outside the window) and rate_texel (the plain form), so a Ramped stands where a
// const float2 * does.
struct Ramped {
    const float2 *sched_geo, *gk;
    float t;
    int ease;
};

__device__ __forceinline__ float2 rate_at(const Ramped &r, uint32_t off)
{
    const float2 s = *(const float2 *)((const char *)r.sched_geo + off);
    return make_float2(ramp(s, r.t, r.ease), ((const float2 *)((const char *)r.gk + off))->y);
}

__device__ __forceinline__ float2 rate_texel(const Ramped &r, size_t i)
{
    return make_float2(ramp(r.sched_geo[i], r.t, r.ease), r.gk[i].y);
}

// A G-only rate tap whose time is not known when its texels are read (vm_carry.hip: one landing point, many to-times):
// the four geometry-schedule texels and the fractions of the chain's rate tap at (x, y), read once; geo_rate ramps the
// four at t and lerps them -- the bits of tapr(.x) on a plane k_rates has ramped at t, and no such plane is stored.
struct GeoTap { float2 s00, s10, s01, s11; float a, b; };

__device__ __forceinline__ GeoTap geo_tap_at(const float2 *sched_geo, int w, int h, int rs, float x, float y)
{
    const Tap t = tap_at(w, h, (size_t)rs, x, y);
    return GeoTap{sched_geo[t.i00], sched_geo[t.i10], sched_geo[t.i01], sched_geo[t.i11], t.a, t.b};
}

__device__ __forceinline__ float geo_rate(const GeoTap &g, float t, int ease)
{
    return lerp2(ramp(g.s00, t, ease), ramp(g.s10, t, ease), ramp(g.s01, t, ease), ramp(g.s11, t, ease), g.a, g.b);
}

} // namespace vm_chain

#endif
