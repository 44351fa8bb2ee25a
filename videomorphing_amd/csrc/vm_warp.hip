// vm_warp.hip -- what the compositor's fixed point knows besides a colour, for gfx950: the two sampling positions of
// every output pixel of kernel_render_halfway_image (Algorithm/render.cu:16-60; UI/RenderWidget.cpp:229-266), how well
// they are founded, and float layers of 1..4 channels carried through the same chain.
//
// The chain itself -- the 21 dependent taps of v (and u), the 32 x 16 tiles, the LDS window with clamped staging, the lean
// global gathers for a tap outside it, and the plain form for fields of 4 GiB and more (VM_RENDER=plain) -- is stated
// once, in vm_chain.h and vm_chain_win.h, for this unit and the renderer (vm_render.hip): k_warp_win includes the window form, k_warp calls chain_plain,
// and each runs one of this unit's tails on what the chain leaves in the pixel.
//
// After the 20 rounds a pixel holds (px, py), the blended v and the p of the round before:
//   map0 = (px - v.x, py - v.y), map1 = (px + v.x, py + v.y)       image pixels, pixel centre i is i
//   resid = fmaxf(|px20 - px19|, |py20 - py19|)                    the move of the last round
//   flags bit 0 / 1: map0 / map1 within [0, w - 1] x [0, h - 1]    (a NaN fails the comparisons)
// A layer is sampled at ((map + lexf) + 0.5f) with tap2's expression and clamps on the lw x lh layer: tight (lexf = 0), where
// the edge texel repeats, or Poisson-extended as the canvases are (vm_layer_ext.hip; lexf = ex).  Tails: the maps kernel four coalesced stores per pixel, the layer kernel 2 x 4 texel gathers of
// C floats (8-byte texels for C = 2, 16-byte for C = 4, three dwords for C = 3: texels stay tight) and one store.
//
// TRANSITION CONTROL (RATES).  The scalar geo_fa / color_fa become per-texel rates in the halfway domain: a
// schedule (t0, t1) per texel and plane (geometry, colour), ramped per texel at the call's time t by the pre-pass k_rates
//   d = t1 - t0;  s = d > 0 ? fminf(fmaxf((t - t0) / d, 0), 1) : (t >= t0 ? 1 : 0);  rate = smooth ? (s s)(3 - 2 s) : s
// into (G, K), one float2 per texel, and sampled at every tap position of the chain with the field taps' index and
// clamp arithmetic in lerp form, r0 = t00 + a (t10 - t00), r1 = t01 + a (t11 - t01), r = r0 + b (r1 - r0) (a constant
// plane gives its value exactly).  g = tapr(G, p) replaces geo_fa round by round, k = tapr(K, p20) replaces color_fa
// in the tail.  The window form stages (G, K) in a third LDS window beside v and u; nothing of the rates is left in
// the uniform instantiations (RATES == false).  A third tail, CANVAS, is the renderer's own: RGB8 from the extended canvases.
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_layer_tap.h"
#include "vm_ramp.h"
#include "vm_warp.h"

namespace {

using namespace vm_chain;

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
    // the layer tail (C >= 1): tight (lh, lw, C), the image at (lexf, lexf) -- (h, w, C) at 0, or the extended (ch, cw, C) at ex
    const float *layer0, *layer1;
    int lw, lh;
    float lexf;
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
        const float3 c0 = tap_rgb(A.ext0, cw, ch, m0x + ex + 0.5f, m0y + ex + 0.5f);
        const float3 c1 = tap_rgb(A.ext1, cw, ch, m1x + ex + 0.5f, m1y + ex + 0.5f);
        rgb8_store(A.rgb + 3 * at, c0, c1, A.color_from, color_fa);
    } else {
        Texel<C> r;
        if (A.color_from == 0) {
            r = tap_layer<C>(A.layer0, A.lw, A.lh, (m0x + A.lexf) + 0.5f, (m0y + A.lexf) + 0.5f);
        } else if (A.color_from == 2) {
            r = tap_layer<C>(A.layer1, A.lw, A.lh, (m1x + A.lexf) + 0.5f, (m1y + A.lexf) + 0.5f);
        } else {
            const Texel<C> c0 = tap_layer<C>(A.layer0, A.lw, A.lh, (m0x + A.lexf) + 0.5f, (m0y + A.lexf) + 0.5f);
            const Texel<C> c1 = tap_layer<C>(A.layer1, A.lw, A.lh, (m1x + A.lexf) + 0.5f, (m1y + A.lexf) + 0.5f);
#pragma unroll
            for (int k = 0; k < C; ++k)
                r.c[k] = c0.c[k] * (1 - color_fa) + c1.c[k] * color_fa;
        }
        texel_store<C>(A.out, at, r);
    }
}

// the plain form: one pixel per thread, every tap a global gather
template <int C, bool RATES> __global__ __launch_bounds__(256) void k_warp(const VmWarpArgs A)
{
    int x, y;
    Landing L;
    if (!chain_plain<RATES>(A.w, A.h, A.rs, A.geo_fa, A.vf, A.uf, A.rates, x, y, L))
        return;
    warp_tail<C, RATES>(A, x, y, L);
}

// the window form: the chain is bound by its taps, not by bytes
template <bool HAS_U, int C, bool RATES> __global__ __launch_bounds__(RW * RH) void k_warp_win(const VmWarpArgs A)
{
    const int w = A.w, h = A.h, rs = A.rs, tiles_x = A.tiles_x, ntiles = A.ntiles;
    const float geo_fa = A.geo_fa;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf, *rates = A.rates;
#include "vm_chain_win.h"
    warp_tail<C, RATES>(A, x, y, L);
}

// (the canvas tail exists under RATES only: the uniform renderer is vm_render.hip)
template <bool RATES> void launch_tail(VmWarpArgs &A, int channels, bool window, hipStream_t s)
{
    for_channels<true, RATES>(channels, [&](auto c) {
        constexpr int C = decltype(c)::value;
        launch_form(window, A.w, A.h, A, k_warp<C, RATES>, k_warp_win<true, C, RATES>, k_warp_win<false, C, RATES>, s);
    });
}

} // namespace

// channels == 0: the maps into map0 / map1 / resid / flags (tight, any may be NULL); 1..4: the layers into out
void vm_launch_warp(int w, int h, int rs, float color_fa, float geo_fa, int color_from, const float2 *v, const float2 *u,
                    float2 *map0, float2 *map1, float *resid, uint8_t *flags, int channels, const float *layer0,
                    const float *layer1, int lw, int lh, float lexf, float *out, hipStream_t s)
{
    VmWarpArgs A{};
    A.w = w; A.h = h; A.rs = rs;
    A.color_fa = color_fa; A.geo_fa = geo_fa; A.color_from = color_from;
    A.vf = v; A.uf = u;
    A.map0 = map0; A.map1 = map1; A.resid = resid; A.flags = flags;
    A.layer0 = layer0; A.layer1 = layer1; A.out = out;
    A.lw = lw; A.lh = lh; A.lexf = lexf;
    launch_tail<false>(A, channels, vm_render_window_form(rs, h), s);
}

void vm_launch_rates(const VmTransition &T, hipStream_t s)
{
    const Grid G = plain_grid(T.w, T.h);
    hipLaunchKernelGGL(k_rates, G.g, G.b, 0, s, T.rates, T.sched_geo, T.sched_color, T.w, T.h, T.rs, T.t, T.ease);
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
    A.lw = T.lw; A.lh = T.lh; A.lexf = T.lexf;
    A.ext0 = T.ext0; A.ext1 = T.ext1; A.ex = T.ex; A.rgb = T.rgb;
    vm_launch_rates(T, s);
    launch_tail<true>(A, T.channels, vm_render_window_form(T.rs, T.h), s);
}
