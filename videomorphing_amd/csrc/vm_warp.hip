// vm_warp.hip -- what the compositor's fixed point knows besides a colour, for gfx950: the two sampling positions of
// every output pixel of kernel_render_halfway_image (Algorithm/render.cu:16-60; UI/RenderWidget.cpp:229-266), how well
// they are founded, and float layers of 1..4 channels carried through the same chain.
//
// THE CHAIN IS RESTATED HERE, NOT SHARED.  k_warp_win walks k_render_win's 21 dependent taps of v (and u) (vm_render.hip)
// with the same float expressions in the same order, the same 32 x 16 tiles, the same LDS window with clamped staging
// and the same lean global gathers for a tap outside the window; k_warp is k_render's plain form (fields of 4 GiB and
// more, VM_RENDER=plain).  A device header that both units include would have to turn the renderer's tap lambda into a
// function of its own, and k_render_win -- the product renderer, the yardstick these kernels are measured beside -- must
// keep its generated code: vm_render.hip is left as it is, and tests/test_gpu_layers.py ties the two statements together
// on the GPU (the maps of this unit, sampled on the host, give vm_render_halfway's bytes).  Who changes the chain in one
// unit changes it in the other.
//
// After the 20 rounds a pixel holds (px, py), the blended v and the p of the round before:
//   map0 = (px - v.x, py - v.y), map1 = (px + v.x, py + v.y)       image pixels, pixel centre i is i
//   resid = fmaxf(|px20 - px19|, |py20 - py19|)                    the move of the last round
//   flags bit 0 / 1: map0 / map1 within [0, w - 1] x [0, h - 1]    (a NaN fails the comparisons)
// A layer is sampled at (map + 0.5f) with tap2's expression and clamps on the w x h layer: no Poisson extension, the
// edge texel repeats.  Tails: the maps kernel four coalesced stores per pixel, the layer kernel 2 x 4 texel gathers of
// C floats (8-byte texels for C = 2, 16-byte for C = 4, three dwords for C = 3: texels stay tight) and one store.
//
// TRANSITION CONTROL (RATES).  The scalar geo_fa / color_fa become per-texel rates in the halfway domain: a
// schedule (t0, t1) per texel and plane (geometry, colour), ramped per texel at the call's time t by the pre-pass k_rates
//   d = t1 - t0;  s = d > 0 ? fminf(fmaxf((t - t0) / d, 0), 1) : (t >= t0 ? 1 : 0);  rate = smooth ? (s s)(3 - 2 s) : s
// into (G, K), one float2 per texel, and sampled at every tap position of the chain with the field taps' index and
// clamp arithmetic in lerp form, r0 = t00 + a (t10 - t00), r1 = t01 + a (t11 - t01), r = r0 + b (r1 - r0) (a constant
// plane gives its value exactly).  g = tapr(G, p) replaces geo_fa round by round, k = tapr(K, p20) replaces color_fa
// in the tail.  The window form stages (G, K) in a third LDS window beside v and u.  The uniform instantiations
// (RATES == false) are the source they were.  A third tail, CANVAS, is the renderer's own: RGB8 from the extended canvases.
#include "vm_warp.h"
#include <cstdlib>
#include <cstring>

namespace {

#ifndef VM_WARP_ITERS
#define VM_WARP_ITERS 20        // render.cu:29
#endif
constexpr int RW = 32, RH = 16, RR = 10, WW = RW + 2 * RR + 1, WH = RH + 2 * RR + 1;   // k_render_win's tile and window

__device__ __forceinline__ int med3_i32(int a, int b, int c)     // median = clamp of a to [b, c] when b <= c
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// what the chain leaves in a pixel
struct Landing {
    float px, py;       // p of round 20
    float lx, ly;       // p of round 19
    float2 v;
    float g, k;         // RATES: the rates at p of round 20
};

// tap2 of vm_render.hip on a field of 64-bit reach
__device__ __forceinline__ float2 tap2(const float2 *__restrict__ img, int w, int h, int rs, float x, float y)
{
    float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    float a = xb - fi, b = yb - fj;
    fi = fminf(fmaxf(fi, -1.0f), (float)w);
    fj = fminf(fmaxf(fj, -1.0f), (float)h);
    int i0 = (int)fi, j0 = (int)fj;
    int i1 = min(max(i0 + 1, 0), w - 1), j1 = min(max(j0 + 1, 0), h - 1);
    i0 = min(max(i0, 0), w - 1);
    j0 = min(max(j0, 0), h - 1);
    float2 t00 = img[(size_t)j0 * rs + i0], t10 = img[(size_t)j0 * rs + i1];
    float2 t01 = img[(size_t)j1 * rs + i0], t11 = img[(size_t)j1 * rs + i1];
    float2 r;
    r.x = (1 - a) * (1 - b) * t00.x + a * (1 - b) * t10.x + (1 - a) * b * t01.x + a * b * t11.x;
    r.y = (1 - a) * (1 - b) * t00.y + a * (1 - b) * t10.y + (1 - a) * b * t01.y + a * b * t11.y;
    return r;
}

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

// tap2's bilinear expression and clamp-to-edge index arithmetic on a tight w x h layer of C channels (64-bit texel
// indices: a 4-channel layer passes 4 GiB before the field does)
template <int C> __device__ __forceinline__ Texel<C> tap_layer(const float *__restrict__ img, int w, int h, float x, float y)
{
    const float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    const float a = xb - fi, b = yb - fj;
    fi = __builtin_amdgcn_fmed3f(fi, -1.0f, (float)w);      // = fminf(fmaxf(fi, -1), w), NaN -> -1 like there
    fj = __builtin_amdgcn_fmed3f(fj, -1.0f, (float)h);
    const int i = (int)fi, j = (int)fj;
    const size_t i0 = (size_t)med3_i32(i, 0, w - 1), i1 = (size_t)med3_i32(i + 1, 0, w - 1);
    const size_t r0 = (size_t)med3_i32(j, 0, h - 1) * (size_t)w, r1 = (size_t)med3_i32(j + 1, 0, h - 1) * (size_t)w;
    const Texel<C> t00 = texel_load<C>(img, r0 + i0), t10 = texel_load<C>(img, r0 + i1);
    const Texel<C> t01 = texel_load<C>(img, r1 + i0), t11 = texel_load<C>(img, r1 + i1);
    Texel<C> r;
#pragma unroll
    for (int k = 0; k < C; ++k)
        r.c[k] = (1 - a) * (1 - b) * t00.c[k] + a * (1 - b) * t10.c[k] + (1 - a) * b * t01.c[k] + a * b * t11.c[k];
    return r;
}

// the renderer's tap_rgb (vm_render.hip) on an RGBA8 canvas, with tap_layer's index arithmetic
__device__ __forceinline__ float3 tap_canvas(const uchar4 *__restrict__ img, int w, int h, float x, float y)
{
    const float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    const float a = xb - fi, b = yb - fj;
    fi = __builtin_amdgcn_fmed3f(fi, -1.0f, (float)w);
    fj = __builtin_amdgcn_fmed3f(fj, -1.0f, (float)h);
    const int i = (int)fi, j = (int)fj;
    const size_t i0 = (size_t)med3_i32(i, 0, w - 1), i1 = (size_t)med3_i32(i + 1, 0, w - 1);
    const size_t r0 = (size_t)med3_i32(j, 0, h - 1) * (size_t)w, r1 = (size_t)med3_i32(j + 1, 0, h - 1) * (size_t)w;
    const uchar4 t00 = img[r0 + i0], t10 = img[r0 + i1], t01 = img[r1 + i0], t11 = img[r1 + i1];
    const float w00 = (1 - a) * (1 - b), w10 = a * (1 - b), w01 = (1 - a) * b, w11 = a * b;
    float3 r;
    r.x = w00 * (float)t00.x + w10 * (float)t10.x + w01 * (float)t01.x + w11 * (float)t11.x;
    r.y = w00 * (float)t00.y + w10 * (float)t10.y + w01 * (float)t01.y + w11 * (float)t11.y;
    r.z = w00 * (float)t00.z + w10 * (float)t10.z + w01 * (float)t01.z + w11 * (float)t11.z;
    return r;
}

constexpr int CANVAS = -1;      // the tail that is neither the maps (0) nor a layer of 1..4 channels

// the arguments of both kernels
struct VmWarpArgs {
    int w, h, rs;
    float color_fa, geo_fa;
    int color_from;
    const float2 *vf, *uf;
    // the maps tail (C == 0): any may be NULL
    float2 *map0, *map1;
    float *resid;
    uint8_t *flags;
    // the layer tail (C >= 1): tight (h, w, C)
    const float *layer0, *layer1;
    float *out;
    int tiles_x, ntiles;
    // transition control (RATES): the call's (G, K) plane, ramped by k_rates, of the field's pitch; the maps tail's (g, k)
    // output (may be NULL)
    const float2 *rates;
    float2 *rates_out;
    // the canvas tail (C == CANVAS): the extended RGBA8 canvases and h rows of w RGB8 pixels, tight
    const uchar4 *ext0, *ext1;
    int ex;
    uint8_t *rgb;
};

// the ramp of one texel's schedule (t0, t1) at time t
__device__ __forceinline__ float ramp(float2 s, float t, int ease)
{
    const float d = s.y - s.x;
    const float r = d > 0.0f ? fminf(fmaxf(__fdiv_rn(t - s.x, d), 0.0f), 1.0f) : (t >= s.x ? 1.0f : 0.0f);
    return ease == VM_EASE_SMOOTH ? (r * r) * (3.0f - 2.0f * r) : r;
}

// the rate texel (G, K) at byte offset `off` of the call's rate plane
template <class Off> __device__ __forceinline__ float2 rate_at(const VmWarpArgs &A, Off off)
{
    return *(const float2 *)((const char *)A.rates + off);
}

// the lerp form of a rate tap: a constant plane gives its value exactly
__device__ __forceinline__ float lerp2(float t00, float t10, float t01, float t11, float a, float b)
{
    const float r0 = t00 + a * (t10 - t00), r1 = t01 + a * (t11 - t01);
    return r0 + b * (r1 - r0);
}

// the pre-pass of a transition call: the two schedule planes ramped per texel into the call's (G, K) plane (all three of
// the field's pitch).  Ramping while staging instead -- every workgroup the cells it stages, a tap outside the window its
// own eight schedule texels -- gives the same bits and was slower.
__global__ __launch_bounds__(256) void k_rates(float2 *__restrict__ rates, const float2 *__restrict__ sched_g,
                                               const float2 *__restrict__ sched_k, int w, int h, int rs, float t, int ease)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h)
        return;
    const size_t at = (size_t)y * rs + x;
    rates[at] = make_float2(ramp(sched_g[at], t, ease), ramp(sched_k[at], t, ease));
}

// the tail of both kernels for pixel (x, y): C == 0 stores the maps, C >= 1 samples and blends the layers, CANVAS the
// extended canvases with the renderer's expressions (vm_render.hip: + ex + 0.5f, + 0.5 in double, truncation)
template <int C, bool RATES> __device__ __forceinline__ void warp_tail(const VmWarpArgs &A, int x, int y, const Landing &L)
{
    const float m0x = L.px - L.v.x, m0y = L.py - L.v.y;
    const float m1x = L.px + L.v.x, m1y = L.py + L.v.y;
    const size_t at = (size_t)y * A.w + x;
    const float color_fa = RATES ? L.k : A.color_fa;
    if constexpr (C == 0) {
        if (A.map0) A.map0[at] = make_float2(m0x, m0y);
        if (A.map1) A.map1[at] = make_float2(m1x, m1y);
        if (A.resid) A.resid[at] = fmaxf(fabsf(L.px - L.lx), fabsf(L.py - L.ly));
        if (A.flags) {
            const float xm = (float)(A.w - 1), ym = (float)(A.h - 1);
            const bool in0 = 0.0f <= m0x && m0x <= xm && 0.0f <= m0y && m0y <= ym;
            const bool in1 = 0.0f <= m1x && m1x <= xm && 0.0f <= m1y && m1y <= ym;
            A.flags[at] = (uint8_t)((in0 ? 1 : 0) | (in1 ? 2 : 0));
        }
        if constexpr (RATES)
            if (A.rates_out) A.rates_out[at] = make_float2(L.g, L.k);
    } else if constexpr (C == CANVAS) {
        const int cw = A.w + 2 * A.ex, ch = A.h + 2 * A.ex, ex = A.ex;
        const float3 c0 = tap_canvas(A.ext0, cw, ch, m0x + ex + 0.5f, m0y + ex + 0.5f);
        const float3 c1 = tap_canvas(A.ext1, cw, ch, m1x + ex + 0.5f, m1y + ex + 0.5f);
        double r, g, b;
        if (A.color_from == 0) {
            r = c0.x + 0.5; g = c0.y + 0.5; b = c0.z + 0.5;
        } else if (A.color_from == 1) {
            r = c0.x * (1 - color_fa) + c1.x * color_fa + 0.5;
            g = c0.y * (1 - color_fa) + c1.y * color_fa + 0.5;
            b = c0.z * (1 - color_fa) + c1.z * color_fa + 0.5;
        } else {
            r = c1.x + 0.5; g = c1.y + 0.5; b = c1.z + 0.5;
        }
        uint8_t *o = A.rgb + 3 * at;
        o[0] = (uint8_t)r;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)b;
    } else {
        Texel<C> r;
        if (A.color_from == 0) {
            r = tap_layer<C>(A.layer0, A.w, A.h, m0x + 0.5f, m0y + 0.5f);
        } else if (A.color_from == 2) {
            r = tap_layer<C>(A.layer1, A.w, A.h, m1x + 0.5f, m1y + 0.5f);
        } else {
            const Texel<C> c0 = tap_layer<C>(A.layer0, A.w, A.h, m0x + 0.5f, m0y + 0.5f);
            const Texel<C> c1 = tap_layer<C>(A.layer1, A.w, A.h, m1x + 0.5f, m1y + 0.5f);
#pragma unroll
            for (int k = 0; k < C; ++k)
                r.c[k] = c0.c[k] * (1 - color_fa) + c1.c[k] * color_fa;
        }
        texel_store<C>(A.out, at, r);
    }
}

// a rate tap (G, K) on the call's rate plane: tap2's index arithmetic, lerp form
__device__ __forceinline__ float2 tapr(const VmWarpArgs &A, float x, float y)
{
    const int w = A.w, h = A.h;
    float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    float a = xb - fi, b = yb - fj;
    fi = fminf(fmaxf(fi, -1.0f), (float)w);
    fj = fminf(fmaxf(fj, -1.0f), (float)h);
    int i0 = (int)fi, j0 = (int)fj;
    int i1 = min(max(i0 + 1, 0), w - 1), j1 = min(max(j0 + 1, 0), h - 1);
    i0 = min(max(i0, 0), w - 1);
    j0 = min(max(j0, 0), h - 1);
    const float2 t00 = rate_at(A, ((size_t)j0 * A.rs + i0) * 8), t10 = rate_at(A, ((size_t)j0 * A.rs + i1) * 8);
    const float2 t01 = rate_at(A, ((size_t)j1 * A.rs + i0) * 8), t11 = rate_at(A, ((size_t)j1 * A.rs + i1) * 8);
    return make_float2(lerp2(t00.x, t10.x, t01.x, t11.x, a, b), lerp2(t00.y, t10.y, t01.y, t11.y, a, b));
}

// ---------------------------------------------------------------------------
// the plain form: k_render's chain (vm_render.hip), one pixel per thread, every tap a global gather
template <int C, bool RATES> __global__ __launch_bounds__(256) void k_warp(const VmWarpArgs A)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.w || y >= A.h)
        return;
    const int w = A.w, h = A.h, rs = A.rs;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf;
    const float alpha = 0.8f;
    float s1 = 2 * A.geo_fa - 1;
    float s2 = 4 * A.geo_fa - 4 * A.geo_fa * A.geo_fa;
    const float qx = (float)x, qy = (float)y;
    Landing L;
    L.px = qx; L.py = qy;
    L.lx = qx; L.ly = qy;
    float2 v = tap2(vf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    float2 u = uf ? tap2(uf, w, h, rs, L.px + 0.5f, L.py + 0.5f) : make_float2(0.0f, 0.0f);
    float2 gk = make_float2(0.0f, 0.0f);
    if constexpr (RATES) gk = tapr(A, L.px + 0.5f, L.py + 0.5f);
    for (int i = 0; i < VM_WARP_ITERS; ++i) {
        L.lx = L.px; L.ly = L.py;
        if constexpr (RATES) {
            s1 = 2 * gk.x - 1;
            s2 = 4 * gk.x - 4 * gk.x * gk.x;
        }
        L.px = qx - s1 * v.x - s2 * u.x;
        L.py = qy - s1 * v.y - s2 * u.y;
        float2 t = tap2(vf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
        v.x = alpha * t.x + (1 - alpha) * v.x;
        v.y = alpha * t.y + (1 - alpha) * v.y;
        if (uf) {
            t = tap2(uf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
            u.x = alpha * t.x + (1 - alpha) * u.x;
            u.y = alpha * t.y + (1 - alpha) * u.y;
        }
        if constexpr (RATES) gk = tapr(A, L.px + 0.5f, L.py + 0.5f);
    }
    L.v = v;
    L.g = gk.x; L.k = gk.y;
    warp_tail<C, RATES>(A, x, y, L);
}

// ---------------------------------------------------------------------------
// the window form: k_render_win's schedule (vm_render.hip) -- the chain is bound by its taps, not by bytes
struct TapIdx {
    uint32_t o00, o10, o01, o11;    // byte offsets of the four texels
};

__device__ __forceinline__ TapIdx tap_index(float x, float y, float fw, float fh, int wm1, int hm1, uint32_t rs)
{
    TapIdx t;
    const float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    fi = __builtin_amdgcn_fmed3f(fi, -1.0f, fw);
    fj = __builtin_amdgcn_fmed3f(fj, -1.0f, fh);
    const int i = (int)fi, j = (int)fj;
    const uint32_t i0 = (uint32_t)med3_i32(i, 0, wm1), i1 = (uint32_t)med3_i32(i + 1, 0, wm1);
    const uint32_t r0 = __umul24((uint32_t)med3_i32(j, 0, hm1), rs), r1 = __umul24((uint32_t)med3_i32(j + 1, 0, hm1), rs);
    t.o00 = (r0 + i0) << 3; t.o10 = (r0 + i1) << 3;
    t.o01 = (r1 + i0) << 3; t.o11 = (r1 + i1) << 3;
    return t;
}

typedef const volatile __attribute__((address_space(3))) unsigned long long *LdsWords;

__device__ __forceinline__ float2 lds8(LdsWords win, uint32_t c)
{
    const unsigned long long q = win[c];
    return make_float2(__uint_as_float((uint32_t)q), __uint_as_float((uint32_t)(q >> 32)));
}

template <bool HAS_U, int C, bool RATES> __global__ __launch_bounds__(RW * RH) void k_warp_win(const VmWarpArgs A)
{
    __shared__ float2 win_v[WH * WW];
    __shared__ float2 win_u[HAS_U ? WH * WW : 1];
    __shared__ float2 win_r[RATES ? WH * WW : 1];      // (G, K) per cell, staged like v
    const int blk = blockIdx.x, per = (A.ntiles + 7) / 8;
    const int tile = (blk % 8) * per + blk / 8;         // contiguous bands of tiles per XCD
    if (tile >= A.ntiles)
        return;                                 // the whole workgroup
    const int w = A.w, h = A.h, rs = A.rs;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf;
    const int bx = (tile % A.tiles_x) * RW, by = (tile / A.tiles_x) * RH;
    const int tid = threadIdx.y * RW + threadIdx.x;
    const float fw = (float)w, fh = (float)h;
    const int wm1 = w - 1, hm1 = h - 1;
    const float alpha = 0.8f;
    float s1 = 2 * A.geo_fa - 1;
    float s2 = 4 * A.geo_fa - 4 * A.geo_fa * A.geo_fa;
    int ox, oy;
    {
        const int cx = min(bx + RW / 2, wm1), cy = min(by + RH / 2, hm1);
        const float2 vc = vf[cy * rs + cx];
        const float2 uc = HAS_U ? uf[cy * rs + cx] : make_float2(0.0f, 0.0f);
        if constexpr (RATES) {             // the window goes where the centre's own rate sends it
            const float gc = rate_at(A, (uint32_t)(cy * rs + cx) << 3).x;
            s1 = 2 * gc - 1;
            s2 = 4 * gc - 4 * gc * gc;
        }
        // (a non-finite or absurd centre puts the window nowhere useful: every tap then takes the global path)
        const float dx = __builtin_amdgcn_fmed3f(s1 * vc.x + s2 * uc.x, -1e6f, 1e6f), dy = __builtin_amdgcn_fmed3f(s1 * vc.y + s2 * uc.y, -1e6f, 1e6f);
        ox = bx - (int)rintf(dx) - RR;
        oy = by - (int)rintf(dy) - RR;
    }
    // staged with CLAMPED source coordinates: every index below is within the field
    for (int i = tid; i < WH * WW; i += RW * RH) {
        const int wy = i / WW, wx = i - wy * WW;
        const int src = min(max(oy + wy, 0), hm1) * rs + min(max(ox + wx, 0), wm1);
        win_v[i] = vf[src];
        if (HAS_U)
            win_u[i] = uf[src];
        if constexpr (RATES)
            win_r[i] = rate_at(A, (uint32_t)src << 3);
    }
    __syncthreads();
    const int x = bx + threadIdx.x, y = by + threadIdx.y;
    if (x >= w || y >= h)
        return;
    const float qx = (float)x, qy = (float)y;
    float px = qx, py = qy, lx = qx, ly = qy;
    float2 v, u = make_float2(0.0f, 0.0f);
    const LdsWords wv = (LdsWords)win_v, wu = (LdsWords)win_u, wr = (LdsWords)win_r;
    // RATES: g of the last tap, and its four K texels and fractions (k is wanted after round 20 only)
    float g = 0.0f, ka = 0.0f, kb = 0.0f, k00 = 0.0f, k10 = 0.0f, k01 = 0.0f, k11 = 0.0f;
    // one tap of v (and u, and the rates) at (px + 0.5, py + 0.5): tap2's expression (the notes on its form: vm_render.hip)
    auto tap = [&](float2 &tv, float2 &tu) {
        const float xb = (px + 0.5f) - 0.5f, yb = (py + 0.5f) - 0.5f;
        const float fi = floorf(xb), fj = floorf(yb);
        const float a = xb - fi, b = yb - fj;
        const uint32_t a0 = (uint32_t)(int)fi - (uint32_t)ox, b0 = (uint32_t)(int)fj - (uint32_t)oy;
        const bool inside = a0 < (uint32_t)(WW - 1) && b0 < (uint32_t)(WH - 1);
        const uint32_t c = inside ? __umul24(b0, (uint32_t)WW) + a0 : 0u;
        float2 t00 = lds8(wv, c), t10 = lds8(wv, c + 1), t01 = lds8(wv, c + WW), t11 = lds8(wv, c + WW + 1);
        float2 u00, u10, u01, u11;
        if (HAS_U) { u00 = lds8(wu, c); u10 = lds8(wu, c + 1); u01 = lds8(wu, c + WW); u11 = lds8(wu, c + WW + 1); }
        float2 r00, r10, r01, r11;
        if constexpr (RATES) { r00 = lds8(wr, c); r10 = lds8(wr, c + 1); r01 = lds8(wr, c + WW); r11 = lds8(wr, c + WW + 1); }
        if (!inside) {
            const TapIdx t = tap_index(px + 0.5f, py + 0.5f, fw, fh, wm1, hm1, (uint32_t)rs);
            const char *bv = (const char *)vf, *bu = (const char *)uf;
            t00 = *(const float2 *)(bv + t.o00); t10 = *(const float2 *)(bv + t.o10);
            t01 = *(const float2 *)(bv + t.o01); t11 = *(const float2 *)(bv + t.o11);
            if (HAS_U) {
                u00 = *(const float2 *)(bu + t.o00); u10 = *(const float2 *)(bu + t.o10);
                u01 = *(const float2 *)(bu + t.o01); u11 = *(const float2 *)(bu + t.o11);
            }
            if constexpr (RATES) {
                r00 = rate_at(A, t.o00); r10 = rate_at(A, t.o10);
                r01 = rate_at(A, t.o01); r11 = rate_at(A, t.o11);
            }
        }
        tv.x = (1 - a) * (1 - b) * t00.x + a * (1 - b) * t10.x + (1 - a) * b * t01.x + a * b * t11.x;
        tv.y = (1 - a) * (1 - b) * t00.y + a * (1 - b) * t10.y + (1 - a) * b * t01.y + a * b * t11.y;
        if (HAS_U) {
            tu.x = (1 - a) * (1 - b) * u00.x + a * (1 - b) * u10.x + (1 - a) * b * u01.x + a * b * u11.x;
            tu.y = (1 - a) * (1 - b) * u00.y + a * (1 - b) * u10.y + (1 - a) * b * u01.y + a * b * u11.y;
        }
        if constexpr (RATES) {
            g = lerp2(r00.x, r10.x, r01.x, r11.x, a, b);
            ka = a; kb = b;
            k00 = r00.y; k10 = r10.y; k01 = r01.y; k11 = r11.y;
        }
    };
    {
        float2 tv, tu;
        tap(tv, tu);
        v = tv;
        if (HAS_U) u = tu;
    }
    for (int i = 0; i < VM_WARP_ITERS; ++i) {
        lx = px; ly = py;
        if constexpr (RATES) {
            s1 = 2 * g - 1;
            s2 = 4 * g - 4 * g * g;
        }
        // (without a path u stays +0 and s2 * u is still subtracted, as k_render_win does)
        px = qx - s1 * v.x - s2 * u.x;
        py = qy - s1 * v.y - s2 * u.y;
        float2 tv, tu;
        tap(tv, tu);
        v.x = alpha * tv.x + (1 - alpha) * v.x;
        v.y = alpha * tv.y + (1 - alpha) * v.y;
        if (HAS_U) {
            u.x = alpha * tu.x + (1 - alpha) * u.x;
            u.y = alpha * tu.y + (1 - alpha) * u.y;
        }
    }
    Landing L;
    L.px = px; L.py = py; L.lx = lx; L.ly = ly; L.v = v;
    L.g = g; L.k = lerp2(k00, k10, k01, k11, ka, kb);
    warp_tail<C, RATES>(A, x, y, L);
}

template <int C, bool RATES> void launch(VmWarpArgs &A, bool window, hipStream_t s)
{
    if (!window) {
        dim3 b(64, 4), g((A.w + 63) / 64, (A.h + 3) / 4);
        hipLaunchKernelGGL((k_warp<C, RATES>), g, b, 0, s, A);
        return;
    }
    A.tiles_x = (A.w + RW - 1) / RW;
    A.ntiles = A.tiles_x * ((A.h + RH - 1) / RH);
    dim3 b(RW, RH), g(((A.ntiles + 7) / 8) * 8);
    if (A.uf)
        hipLaunchKernelGGL((k_warp_win<true, C, RATES>), g, b, 0, s, A);
    else
        hipLaunchKernelGGL((k_warp_win<false, C, RATES>), g, b, 0, s, A);
}

template <bool RATES> void launch_tail(VmWarpArgs &A, int channels, bool window, hipStream_t s)
{
    switch (channels) {
    case 0: launch<0, RATES>(A, window, s); break;
    case 1: launch<1, RATES>(A, window, s); break;
    case 2: launch<2, RATES>(A, window, s); break;
    case 3: launch<3, RATES>(A, window, s); break;
    case 4: launch<4, RATES>(A, window, s); break;
    default:
        if constexpr (RATES) launch<CANVAS, RATES>(A, window, s);
        break;
    }
}

// the renderer's switch (both take their plain forms), and what the window kernel can address: the field's texels by
// 32-bit byte offsets, rows multiplied in 24 bits
bool window_form(int rs, int h)
{
    static const char *mode = getenv("VM_RENDER");
    static const bool plain = mode && !strcmp(mode, "plain");
    const bool small = (uint64_t)rs * (uint64_t)h * 8ull < (1ull << 32) && rs < (1 << 24) && h < (1 << 24);
    return small && !plain;
}

} // namespace

// channels == 0: the maps into map0 / map1 / resid / flags (tight, any may be NULL); 1..4: the layers into out
void vm_launch_warp(int w, int h, int rs, float color_fa, float geo_fa, int color_from, const float2 *v, const float2 *u,
                    float2 *map0, float2 *map1, float *resid, uint8_t *flags, int channels, const float *layer0,
                    const float *layer1, float *out, hipStream_t s)
{
    VmWarpArgs A{};
    A.w = w; A.h = h; A.rs = rs;
    A.color_fa = color_fa; A.geo_fa = geo_fa; A.color_from = color_from;
    A.vf = v; A.uf = u;
    A.map0 = map0; A.map1 = map1; A.resid = resid; A.flags = flags;
    A.layer0 = layer0; A.layer1 = layer1; A.out = out;
    launch_tail<false>(A, channels, window_form(rs, h), s);
}

void vm_launch_transition(const VmTransition &T, hipStream_t s)
{
    VmWarpArgs A{};
    A.w = T.w; A.h = T.h; A.rs = T.rs;
    A.color_from = T.color_from;
    A.vf = T.v; A.uf = T.u;
    A.rates = T.rates;
    A.map0 = T.map0; A.map1 = T.map1; A.resid = T.resid; A.flags = T.flags; A.rates_out = T.rates_out;
    A.layer0 = T.layer0; A.layer1 = T.layer1; A.out = T.out;
    A.ext0 = T.ext0; A.ext1 = T.ext1; A.ex = T.ex; A.rgb = T.rgb;
    dim3 b(64, 4), g((T.w + 63) / 64, (T.h + 3) / 4);
    hipLaunchKernelGGL(k_rates, g, b, 0, s, T.rates, T.sched_geo, T.sched_color, T.w, T.h, T.rs, T.t, T.ease);
    launch_tail<true>(A, T.channels, window_form(T.rs, T.h), s);
}
