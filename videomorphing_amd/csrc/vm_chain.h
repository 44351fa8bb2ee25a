// vm_chain.h -- the compositor's fixed-point chain (kernel_render_halfway_image, Algorithm/render.cu:16-60), stated once
// for the units that walk it: vm_render.hip (RGB8 from the extended canvases), vm_warp.hip (sampling maps, float
// layers, transition control), vm_shutter.hip (both tails over the sample times of a shutter), vm_tshutter.hip (the same under a schedule) and vm_viewport.hip (both tails from the sub-sample points of a viewport), vm_vshutter.hip (a viewport over either shutter), vm_carry.hip (the landing carried to other times), vm_multiband.hip (the two plates kept apart for a blend band by band).  A kernel walks the window form (the product path: taps served from an LDS window;
// vm_chain_win.h, included in the kernel's body) or calls chain_plain (VM_RENDER=plain, and fields of 4 GiB and more),
// returns if the chain gave its thread no pixel, and runs its own tail on the Landing.  Everything is float32 in tap2's
// expressions and order; the units are compiled with -ffp-contract=off.  Every function here is inlined into the kernel
// that calls it.
#ifndef VM_CHAIN_H
#define VM_CHAIN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef VM_RENDER_ITERS
#define VM_RENDER_ITERS 20      // render.cu:29 (anything else: a timing experiment)
#endif
#ifndef VM_RENDER_RR
#define VM_RENDER_RR 10
#endif
#ifndef VM_RENDER_RH
#define VM_RENDER_RH 16     // 32 x 16 pixels per workgroup: 3.8 staged cells per pixel (8 rows: 6.0; 63.0 -> 60.7 us per frame)
#endif

namespace vm_chain {

// the window form's tile (RW x RH pixels per workgroup), its margin RR and the staged window of WW x WH cells
constexpr int RW = 32, RH = VM_RENDER_RH, RR = VM_RENDER_RR, WW = RW + 2 * RR + 1, WH = RH + 2 * RR + 1;

// what the chain leaves in a pixel
struct Landing {
    float px, py;       // p of round 20
    float lx, ly;       // p of round 19
    float2 v;
    float g, k;         // RATES: the rates at p of round 20
    float2 u;           // the damped path (zero without one): read by vm_carry.hip only, dead in every other tail
};

__device__ __forceinline__ int med3_i32(int a, int b, int c)     // median = clamp of a to [b, c] when b <= c
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// where a bilinear tap at (x, y) reads a w x h image of row stride rs: its fractions and the 64-bit indices of its four
// texels, clamped to the edge (the plain kernels exist for fields of 4 GiB and more).  The clamp of floor() to [-1, w]
// is one v_med3_f32 (= fminf(fmaxf(fi, -1), w), NaN -> -1 like there), the clamps of i0 / i0 + 1 to [0, w - 1] one
// v_med3_i32 each.
struct Tap { float a, b; size_t i00, i10, i01, i11; };

__device__ __forceinline__ Tap tap_at(int w, int h, size_t rs, float x, float y)
{
    Tap t;
    const float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    t.a = xb - fi; t.b = yb - fj;
    fi = __builtin_amdgcn_fmed3f(fi, -1.0f, (float)w);
    fj = __builtin_amdgcn_fmed3f(fj, -1.0f, (float)h);
    const int i = (int)fi, j = (int)fj;
    const size_t i0 = (size_t)med3_i32(i, 0, w - 1), i1 = (size_t)med3_i32(i + 1, 0, w - 1);
    const size_t r0 = (size_t)med3_i32(j, 0, h - 1) * rs, r1 = (size_t)med3_i32(j + 1, 0, h - 1) * rs;
    t.i00 = r0 + i0; t.i10 = r0 + i1;
    t.i01 = r1 + i0; t.i11 = r1 + i1;
    return t;
}

// one bilinear tap of a pitched float2 field: render.cu's expression, from left to right
__device__ __forceinline__ float2 tap2(const float2 *__restrict__ img, int w, int h, int rs, float x, float y)
{
    const Tap t = tap_at(w, h, (size_t)rs, x, y);
    const float a = t.a, b = t.b;
    const float2 t00 = img[t.i00], t10 = img[t.i10], t01 = img[t.i01], t11 = img[t.i11];
    float2 r;
    r.x = (1 - a) * (1 - b) * t00.x + a * (1 - b) * t10.x + (1 - a) * b * t01.x + a * b * t11.x;
    r.y = (1 - a) * (1 - b) * t00.y + a * (1 - b) * t10.y + (1 - a) * b * t01.y + a * b * t11.y;
    return r;
}

// the lerp form of a rate tap: a constant plane gives its value exactly
__device__ __forceinline__ float lerp2(float t00, float t10, float t01, float t11, float a, float b)
{
    const float r0 = t00 + a * (t10 - t00), r1 = t01 + a * (t11 - t01);
    return r0 + b * (r1 - r0);
}

// a rate tap (G, K) on a transition call's rate plane (vm_warp.hip): tap2's index arithmetic, lerp form
__device__ __forceinline__ float2 tapr(const float2 *rates, int w, int h, int rs, float x, float y)
{
    const Tap t = tap_at(w, h, (size_t)rs, x, y);
    const float2 t00 = rates[t.i00], t10 = rates[t.i10], t01 = rates[t.i01], t11 = rates[t.i11];
    return make_float2(lerp2(t00.x, t10.x, t01.x, t11.x, t.a, t.b), lerp2(t00.y, t10.y, t01.y, t11.y, t.a, t.b));
}

// the same on rates that are no stored plane: anything with a rate_texel(rates, 64-bit index) of its own (vm_ramp.h)
template <class Rates> __device__ __forceinline__ float2 tapr(const Rates &rates, int w, int h, int rs, float x, float y)
{
    const Tap t = tap_at(w, h, (size_t)rs, x, y);
    const float2 t00 = rate_texel(rates, t.i00), t10 = rate_texel(rates, t.i10), t01 = rate_texel(rates, t.i01), t11 = rate_texel(rates, t.i11);
    return make_float2(lerp2(t00.x, t10.x, t01.x, t11.x, t.a, t.b), lerp2(t00.y, t10.y, t01.y, t11.y, t.a, t.b));
}

// ---------------------------------------------------------------------------
// the plain form: pixel (x, y) of a 64 x 4 block, every tap a global gather.  RATES (transition control):
// g = tapr(G, p) replaces geo_fa round by round, k = tapr(K, p20) is left for the tail.  false: no pixel for this thread.
// Rates: const float2 * (or nullptr without RATES), or what the second tapr takes.
template <bool RATES, class Rates>
__device__ __forceinline__ bool chain_plain(int w, int h, int rs, float geo_fa, const float2 *vf,
                                            const float2 *uf, Rates rates, int &x, int &y, Landing &L)
{
    x = blockIdx.x * 64 + threadIdx.x; y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h)
        return false;
    const float alpha = 0.8f;
    float s1 = 2 * geo_fa - 1;
    float s2 = 4 * geo_fa - 4 * geo_fa * geo_fa;
    const float qx = (float)x, qy = (float)y;
    L.px = qx; L.py = qy;
    L.lx = qx; L.ly = qy;
    float2 v = tap2(vf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    float2 u = uf ? tap2(uf, w, h, rs, L.px + 0.5f, L.py + 0.5f) : make_float2(0.0f, 0.0f);
    float2 gk = make_float2(0.0f, 0.0f);
    if constexpr (RATES) gk = tapr(rates, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    for (int i = 0; i < VM_RENDER_ITERS; ++i) {
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
        if (uf) {       // (a zero path stays zero: alpha * 0 + (1 - alpha) * 0)
            t = tap2(uf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
            u.x = alpha * t.x + (1 - alpha) * u.x;
            u.y = alpha * t.y + (1 - alpha) * u.y;
        }
        if constexpr (RATES) gk = tapr(rates, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    }
    L.v = v; L.u = u;
    L.g = gk.x; L.k = gk.y;
    return true;
}

// the plain form from any point q of the halfway domain in the place of the pixel (a pixel's centre i is q = i; the
// viewport kernels of vm_viewport.hip start between pixels, and own their output grid): chain_plain's statements, stated
// beside it and not under it, because chain_plain's callers compile to other (equivalent) code once it calls this.
template <bool RATES, class Rates>
__device__ __forceinline__ void chain_plain_from(int w, int h, int rs, float geo_fa, const float2 *vf, const float2 *uf,
                                                 Rates rates, const float qx, const float qy, Landing &L)
{
    const float alpha = 0.8f;
    float s1 = 2 * geo_fa - 1;
    float s2 = 4 * geo_fa - 4 * geo_fa * geo_fa;
    L.px = qx; L.py = qy;
    L.lx = qx; L.ly = qy;
    float2 v = tap2(vf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    float2 u = uf ? tap2(uf, w, h, rs, L.px + 0.5f, L.py + 0.5f) : make_float2(0.0f, 0.0f);
    float2 gk = make_float2(0.0f, 0.0f);
    if constexpr (RATES) gk = tapr(rates, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    for (int i = 0; i < VM_RENDER_ITERS; ++i) {
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
        if (uf) {       // (a zero path stays zero: alpha * 0 + (1 - alpha) * 0)
            t = tap2(uf, w, h, rs, L.px + 0.5f, L.py + 0.5f);
            u.x = alpha * t.x + (1 - alpha) * u.x;
            u.y = alpha * t.y + (1 - alpha) * u.y;
        }
        if constexpr (RATES) gk = tapr(rates, w, h, rs, L.px + 0.5f, L.py + 0.5f);
    }
    L.v = v; L.u = u;
    L.g = gk.x; L.k = gk.y;
}

// ---------------------------------------------------------------------------
// Lean index arithmetic of a tap in the window form (the float results are tap2's expressions in tap2's order): tap_at's
// clamps, row offsets by 24-bit multiplies (full rate), texel addresses as 32-bit byte offsets from a scalar base (no
// sign extension, no 64-bit address arithmetic per texel): the launchers take the window form only when the field is
// smaller than 4 GiB (vm_render_window_form, vm_warp.h).  SHIFT: log2 of the texel's bytes.
struct TapIdx { uint32_t o00, o10, o01, o11; };      // byte offsets of the four texels

template <int SHIFT> __device__ __forceinline__ TapIdx tap_index(float x, float y, float fw, float fh, int wm1, int hm1, uint32_t rs)
{
    TapIdx t;
    const float xb = x - 0.5f, yb = y - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    fi = __builtin_amdgcn_fmed3f(fi, -1.0f, fw);
    fj = __builtin_amdgcn_fmed3f(fj, -1.0f, fh);
    const int i = (int)fi, j = (int)fj;
    const uint32_t i0 = (uint32_t)med3_i32(i, 0, wm1), i1 = (uint32_t)med3_i32(i + 1, 0, wm1);
    const uint32_t r0 = __umul24((uint32_t)med3_i32(j, 0, hm1), rs), r1 = __umul24((uint32_t)med3_i32(j + 1, 0, hm1), rs);
    t.o00 = (r0 + i0) << SHIFT; t.o10 = (r0 + i1) << SHIFT;
    t.o01 = (r1 + i0) << SHIFT; t.o11 = (r1 + i1) << SHIFT;
    return t;
}

// the rate texel (G, K) at a 32-bit byte offset of the rate plane
__device__ __forceinline__ float2 rate_at(const float2 *rates, uint32_t off) { return *(const float2 *)((const char *)rates + off); }

typedef const volatile __attribute__((address_space(3))) unsigned long long *LdsWords;

__device__ __forceinline__ float2 lds8(LdsWords win, uint32_t c)
{
    const unsigned long long q = win[c];
    return make_float2(__uint_as_float((uint32_t)q), __uint_as_float((uint32_t)(q >> 32)));
}

// ---------------------------------------------------------------------------
// The window form is vm_chain_win.h: a statement sequence a kernel includes in its body, not a function (see there).

// ---------------------------------------------------------------------------
// the canvas taps: tap2's weights on an RGBA8 canvas (uchar -> float is exact).  tap_rgb indexes texels in 64 bits;
// tap_rgb_lean by 32-bit byte offsets and 24-bit row multiplies, for a canvas below 4 GiB.
// (texels by reference: taken by value, the compiler schedules the chain's loop before this differently)
__device__ __forceinline__ float3 rgb_blend(const uchar4 &t00, const uchar4 &t10, const uchar4 &t01, const uchar4 &t11, float a, float b)
{
    const float w00 = (1 - a) * (1 - b), w10 = a * (1 - b), w01 = (1 - a) * b, w11 = a * b;
    float3 r;
    r.x = w00 * (float)t00.x + w10 * (float)t10.x + w01 * (float)t01.x + w11 * (float)t11.x;
    r.y = w00 * (float)t00.y + w10 * (float)t10.y + w01 * (float)t01.y + w11 * (float)t11.y;
    r.z = w00 * (float)t00.z + w10 * (float)t10.z + w01 * (float)t01.z + w11 * (float)t11.z;
    return r;
}

__device__ __forceinline__ float3 tap_rgb(const uchar4 *__restrict__ img, int w, int h, float x, float y)
{
    const Tap t = tap_at(w, h, (size_t)w, x, y);
    return rgb_blend(img[t.i00], img[t.i10], img[t.i01], img[t.i11], t.a, t.b);
}

__device__ __forceinline__ float3 tap_rgb_lean(const uchar4 *__restrict__ img, float fw, float fh, int wm1, int hm1, uint32_t w, float x,
                                               float y)
{
    const float xb = x - 0.5f, yb = y - 0.5f;
    const TapIdx t = tap_index<2>(x, y, fw, fh, wm1, hm1, w);
    const char *base = (const char *)img;
    return rgb_blend(*(const uchar4 *)(base + t.o00), *(const uchar4 *)(base + t.o10), *(const uchar4 *)(base + t.o01),
                     *(const uchar4 *)(base + t.o11), xb - floorf(xb), yb - floorf(yb));
}

// the renderer's RGB8 tail into o[0..2]: the blend by color_from, + 0.5 in double, make_uchar3's truncation
// (render.cu:49-56)
__device__ __forceinline__ void rgb8_store(uint8_t *o, float3 c0, float3 c1, int color_from, float color_fa)
{
    double r, g, b;
    if (color_from == 0) {
        r = c0.x + 0.5; g = c0.y + 0.5; b = c0.z + 0.5;
    } else if (color_from == 1) {
        r = c0.x * (1 - color_fa) + c1.x * color_fa + 0.5;
        g = c0.y * (1 - color_fa) + c1.y * color_fa + 0.5;
        b = c0.z * (1 - color_fa) + c1.z * color_fa + 0.5;
    } else {
        r = c1.x + 0.5; g = c1.y + 0.5; b = c1.z + 0.5;
    }
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)g;
    o[2] = (uint8_t)b;
}

} // namespace vm_chain

#endif
