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
};

// the tail of both kernels for pixel (x, y): C == 0 stores the maps, C >= 1 samples and blends the layers
template <int C> __device__ __forceinline__ void warp_tail(const VmWarpArgs &A, int x, int y, const Landing &L)
{
    const float m0x = L.px - L.v.x, m0y = L.py - L.v.y;
    const float m1x = L.px + L.v.x, m1y = L.py + L.v.y;
    const size_t at = (size_t)y * A.w + x;
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
                r.c[k] = c0.c[k] * (1 - A.color_fa) + c1.c[k] * A.color_fa;
        }
        texel_store<C>(A.out, at, r);
    }
}

// ---------------------------------------------------------------------------
// the plain form: k_render's chain (vm_render.hip), one pixel per thread, every tap a global gather
template <int C> __global__ __launch_bounds__(256) void k_warp(const VmWarpArgs A)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.w || y >= A.h)
        return;
    const int w = A.w, h = A.h, rs = A.rs;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf;
    const float alpha = 0.8f;
    const float s1 = 2 * A.geo_fa - 1;
    const float s2 = 4 * A.geo_fa - 4 * A.geo_fa * A.geo_fa;
    const float qx = (float)x, qy = (float)y;
    Landing L;
    L.px = qx; L.py = qy;
    L.lx = qx; L.ly = qy;
    float2 v = tap2(vf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    float2 u = uf ? tap2(uf, w, h, rs, L.px + 0.5f, L.py + 0.5f) : make_float2(0.0f, 0.0f);
    for (int i = 0; i < VM_WARP_ITERS; ++i) {
        L.lx = L.px; L.ly = L.py;
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
    }
    L.v = v;
    warp_tail<C>(A, x, y, L);
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

template <bool HAS_U, int C> __global__ __launch_bounds__(RW * RH) void k_warp_win(const VmWarpArgs A)
{
    __shared__ float2 win_v[WH * WW];
    __shared__ float2 win_u[HAS_U ? WH * WW : 1];
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
    const float s1 = 2 * A.geo_fa - 1;
    const float s2 = 4 * A.geo_fa - 4 * A.geo_fa * A.geo_fa;
    int ox, oy;
    {
        const int cx = min(bx + RW / 2, wm1), cy = min(by + RH / 2, hm1);
        const float2 vc = vf[cy * rs + cx];
        const float2 uc = HAS_U ? uf[cy * rs + cx] : make_float2(0.0f, 0.0f);
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
    }
    __syncthreads();
    const int x = bx + threadIdx.x, y = by + threadIdx.y;
    if (x >= w || y >= h)
        return;
    const float qx = (float)x, qy = (float)y;
    float px = qx, py = qy, lx = qx, ly = qy;
    float2 v, u = make_float2(0.0f, 0.0f);
    const LdsWords wv = (LdsWords)win_v, wu = (LdsWords)win_u;
    // one tap of v (and u) at (px + 0.5, py + 0.5): tap2's expression (the notes on its form: vm_render.hip)
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
        if (!inside) {
            const TapIdx t = tap_index(px + 0.5f, py + 0.5f, fw, fh, wm1, hm1, (uint32_t)rs);
            const char *bv = (const char *)vf, *bu = (const char *)uf;
            t00 = *(const float2 *)(bv + t.o00); t10 = *(const float2 *)(bv + t.o10);
            t01 = *(const float2 *)(bv + t.o01); t11 = *(const float2 *)(bv + t.o11);
            if (HAS_U) {
                u00 = *(const float2 *)(bu + t.o00); u10 = *(const float2 *)(bu + t.o10);
                u01 = *(const float2 *)(bu + t.o01); u11 = *(const float2 *)(bu + t.o11);
            }
        }
        tv.x = (1 - a) * (1 - b) * t00.x + a * (1 - b) * t10.x + (1 - a) * b * t01.x + a * b * t11.x;
        tv.y = (1 - a) * (1 - b) * t00.y + a * (1 - b) * t10.y + (1 - a) * b * t01.y + a * b * t11.y;
        if (HAS_U) {
            tu.x = (1 - a) * (1 - b) * u00.x + a * (1 - b) * u10.x + (1 - a) * b * u01.x + a * b * u11.x;
            tu.y = (1 - a) * (1 - b) * u00.y + a * (1 - b) * u10.y + (1 - a) * b * u01.y + a * b * u11.y;
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
    warp_tail<C>(A, x, y, L);
}

template <int C> void launch(VmWarpArgs &A, bool window, hipStream_t s)
{
    if (!window) {
        dim3 b(64, 4), g((A.w + 63) / 64, (A.h + 3) / 4);
        hipLaunchKernelGGL(k_warp<C>, g, b, 0, s, A);
        return;
    }
    A.tiles_x = (A.w + RW - 1) / RW;
    A.ntiles = A.tiles_x * ((A.h + RH - 1) / RH);
    dim3 b(RW, RH), g(((A.ntiles + 7) / 8) * 8);
    if (A.uf)
        hipLaunchKernelGGL((k_warp_win<true, C>), g, b, 0, s, A);
    else
        hipLaunchKernelGGL((k_warp_win<false, C>), g, b, 0, s, A);
}

} // namespace

// channels == 0: the maps into map0 / map1 / resid / flags (tight, any may be NULL); 1..4: the layers into out
void vm_launch_warp(int w, int h, int rs, float color_fa, float geo_fa, int color_from, const float2 *v, const float2 *u,
                    float2 *map0, float2 *map1, float *resid, uint8_t *flags, int channels, const float *layer0,
                    const float *layer1, float *out, hipStream_t s)
{
    static const char *mode = getenv("VM_RENDER");
    static const bool plain = mode && !strcmp(mode, "plain");      // the renderer's switch: both take their plain forms
    // the window kernel addresses the field's texels by 32-bit byte offsets and multiplies rows in 24 bits
    const bool small = (uint64_t)rs * (uint64_t)h * 8ull < (1ull << 32) && rs < (1 << 24) && h < (1 << 24);
    VmWarpArgs A{};
    A.w = w; A.h = h; A.rs = rs;
    A.color_fa = color_fa; A.geo_fa = geo_fa; A.color_from = color_from;
    A.vf = v; A.uf = u;
    A.map0 = map0; A.map1 = map1; A.resid = resid; A.flags = flags;
    A.layer0 = layer0; A.layer1 = layer1; A.out = out;
    const bool window = small && !plain;
    switch (channels) {
    case 0: launch<0>(A, window, s); break;
    case 1: launch<1>(A, window, s); break;
    case 2: launch<2>(A, window, s); break;
    case 3: launch<3>(A, window, s); break;
    default: launch<4>(A, window, s); break;
    }
}
