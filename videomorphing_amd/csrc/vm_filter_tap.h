// vm_filter_tap.h -- the cubic tail of the filtered viewport calls, for vm_filter.hip: add_sample_cubic<C>
// beside add_sample<C> of vm_shutter_tail.h, and store_mean's store with the clamp a cubic filter's overshoot asks for.
// The chain is not touched: only the taps that read picture content -- a canvas, a layer -- go through the filter.
//
// A cubic tap reads a W x H image at (x, y), the coordinates tap_at takes.  In float32, without contraction, in this order:
//   xb = x - 0.5f;  fi = floorf(xb);  a = xb - fi;  fi = fminf(fmaxf(fi, -2.0f), (float)W + 1.0f);  i = (int)fi
//   columns  c_k = clamp(i + k, 0, W - 1),  k = -1, 0, 1, 2                 (rows r_m from y, b, H likewise)
//   inner(d) = ((p3 * d + p2) * d) * d + p0            outer(d) = ((q3 * d + q2) * d + q1) * d + q0
//   wx_-1 = outer(1.0f + a)   wx_0 = inner(a)   wx_1 = inner(1.0f - a)   wx_2 = outer(2.0f - a)     (wy from b likewise)
//   row_m = ((wx_-1 * t(c_-1, r_m) + wx_0 * t(c_0, r_m)) + wx_1 * t(c_1, r_m)) + wx_2 * t(c_2, r_m)
//   value = ((wy_-1 * row_-1 + wy_0 * row_0) + wy_1 * row_1) + wy_2 * row_2
// per channel (uchar -> float is exact).  The float clamp stands before the conversion to int: whatever x is -- NaN
// (fmaxf gives -2), +-inf, 1e30 -- i lies in [-2, W + 1] and every column in [0, W - 1].  No tap reads outside the image.
#ifndef VM_FILTER_TAP_H
#define VM_FILTER_TAP_H

#include "vm_chain.h"
#include "vm_layer_tap.h"
#include "vm_shutter_tail.h"

namespace vm_chain {

// the two polynomials of one cubic filter (vm_filter.h)
struct Cubic { float p3, p2, p0, q3, q2, q1, q0; };

__device__ __forceinline__ float cubic_inner(const Cubic &K, float d) { return ((K.p3 * d + K.p2) * d) * d + K.p0; }
__device__ __forceinline__ float cubic_outer(const Cubic &K, float d) { return ((K.q3 * d + K.q2) * d + K.q1) * d + K.q0; }

// one axis of a cubic tap on n texels: the fraction, and the clamped index of the texel the sample lies behind
struct CubicAxis { float a; int i; };

__device__ __forceinline__ CubicAxis cubic_axis(int n, float x)
{
    CubicAxis t;
    const float xb = x - 0.5f;
    float fi = floorf(xb);
    t.a = xb - fi;
    fi = fminf(fmaxf(fi, -2.0f), (float)n + 1.0f);
    t.i = (int)fi;
    return t;
}

// texel k = -1 .. 2 of an axis, clamped to the image, and its weight
__device__ __forceinline__ int cubic_texel(int i, int k, int n) { return med3_i32(i + k, 0, n - 1); }

__device__ __forceinline__ float cubic_weight(const Cubic &K, float a, int k)
{
    return k == -1 ? cubic_outer(K, 1.0f + a) : k == 0 ? cubic_inner(K, a) : k == 1 ? cubic_inner(K, 1.0f - a) : cubic_outer(K, 2.0f - a);
}

// The cubic tap of a w x h image of N channels; fetch_row(first texel of the row, the four columns, float (&t)[4][N]) reads
// one row's four texels (64-bit texel indices, as tap_layer and tap_rgb).  The rows are walked one after the other: row
// m's texels are summed into the value before row m + 1 is fetched -- the row's index j and its fraction b pass through
// a statement that stands behind the one the value passes through, as add_sample sequences its two sides, so that the
// next row's index and weight are formed there and not ahead.  Four texels and one row sum per channel are live at a
// time; left to itself the compiler fetches all sixteen texels at once and holds the four row weights and indices beside
// them, which costs the window kernels their eighth wave.
template <int N, class FetchRow>
__device__ __forceinline__ void tap_cubic(FetchRow fetch_row, int w, int h, const Cubic &K, float x, float y, float (&r)[N])
{
    const CubicAxis X = cubic_axis(w, x), Y = cubic_axis(h, y);
    float wx[4];
    uint32_t cx[4];                     // (unsigned: widened to a texel index without a register for the sign)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wx[k] = cubic_weight(K, X.a, k - 1);
        cx[k] = (uint32_t)cubic_texel(X.i, k - 1, w);
    }
    int j = Y.i;
    float b = Y.a;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const size_t row = (size_t)cubic_texel(j, m - 1, h) * (size_t)w;
        const float wy = cubic_weight(K, b, m - 1);
        float t[4][N];
        fetch_row(row, cx, t);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float s = ((wx[0] * t[0][k] + wx[1] * t[1][k]) + wx[2] * t[2][k]) + wx[3] * t[3][k];
            r[k] = m == 0 ? wy * s : r[k] + wy * s;
        }
        if (m < 3) {
#pragma unroll
            for (int k = 0; k < N; ++k)
                asm volatile("" : "+v"(r[k]));
            asm volatile("" : "+v"(j), "+v"(b));
        }
    }
}

// the cubic tap of a tight w x h layer of C interleaved channels
template <int C> __device__ __forceinline__ Texel<C> tap_layer_cubic(const float *__restrict__ img, int w, int h, const Cubic &K, float x, float y)
{
    Texel<C> r;
    tap_cubic<C>([&](size_t row, const uint32_t (&cx)[4], float (&t)[4][C]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const Texel<C> q = texel_load<C>(img, row + cx[i]);
#pragma unroll
            for (int k = 0; k < C; ++k)
                t[i][k] = q.c[k];
        }
    }, w, h, K, x, y, r.c);
    return r;
}

// four RGBA8 texels in one load: 16 bytes on a texel's alignment
typedef uint32_t CanvasRow __attribute__((ext_vector_type(4), aligned(4)));

// the cubic tap of an RGBA8 canvas: three channels, uchar -> float exact.  Where none of the four columns clamps -- all of
// a picture but its two edge columns -- a row's texels are 16 contiguous bytes and come in one load; the four-load path
// serves the rest.  Measured at 1080p (profiles/filtered.md): the RGB8 calls cost 1.31 x the bilinear ones with four loads
// per row and 1.20 x with one (the identity viewport), 1.27 x and 1.01 x as a half-size proxy.
__device__ __forceinline__ float3 tap_rgb_cubic(const uchar4 *__restrict__ img, int w, int h, const Cubic &K, float x, float y)
{
    float r[3];
    tap_cubic<3>([&](size_t row, const uint32_t (&cx)[4], float (&t)[4][3]) {
        uint32_t q[4];
        if (cx[3] - cx[0] == 3u) {
            const CanvasRow c = *(const CanvasRow *)(img + (row + cx[0]));
            q[0] = c.x; q[1] = c.y; q[2] = c.z; q[3] = c.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                q[i] = *(const uint32_t *)(img + (row + cx[i]));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            t[i][0] = (float)(q[i] & 255u); t[i][1] = (float)((q[i] >> 8) & 255u); t[i][2] = (float)((q[i] >> 16) & 255u);
        }
    }, w, h, K, x, y, r);
    return make_float3(r[0], r[1], r[2]);
}

// acc += c_s: add_sample with the cubic taps.  Args: add_sample's, and the filter's p3 .. q0 (taken from their scalar
// registers anew in every round, as per_sample says).  Side 1 is tapped after side 0 is summed, for every channel count.
template <int C, class Args> __device__ __forceinline__ void add_sample_cubic(const Args &A, const Landing &L, float color_fa, float (&acc)[NACC<C>])
{
    const Cubic K{per_sample(A.p3), per_sample(A.p2), per_sample(A.p0), per_sample(A.q3), per_sample(A.q2), per_sample(A.q1), per_sample(A.q0)};
    const float m0x = L.px - L.v.x, m0y = L.py - L.v.y;
    float m1x = L.px + L.v.x, m1y = L.py + L.v.y;
    if constexpr (C == CANVAS) {
        const int cw = per_sample(A.w + 2 * A.ex), ch = per_sample(A.h + 2 * A.ex), ex = per_sample(A.ex);
        float3 c;
        if (A.color_from == 0) {
            c = tap_rgb_cubic(A.ext0, cw, ch, K, m0x + ex + 0.5f, m0y + ex + 0.5f);
        } else if (A.color_from == 2) {
            c = tap_rgb_cubic(A.ext1, cw, ch, K, m1x + ex + 0.5f, m1y + ex + 0.5f);
        } else {
            float3 c0 = tap_rgb_cubic(A.ext0, cw, ch, K, m0x + ex + 0.5f, m0y + ex + 0.5f);
            asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z));
            asm volatile("" : "+v"(m1x), "+v"(m1y));
            const float3 c1 = tap_rgb_cubic(A.ext1, cw, ch, K, m1x + ex + 0.5f, m1y + ex + 0.5f);
            c.x = c0.x * (1 - color_fa) + c1.x * color_fa;
            c.y = c0.y * (1 - color_fa) + c1.y * color_fa;
            c.z = c0.z * (1 - color_fa) + c1.z * color_fa;
        }
        acc[0] = acc[0] + c.x; acc[1] = acc[1] + c.y; acc[2] = acc[2] + c.z;
    } else {
        const int lw = per_sample(A.lw), lh = per_sample(A.lh);
        const float lexf = per_sample(A.lexf);
        Texel<C> r;
        if (A.color_from == 0) {
            r = tap_layer_cubic<C>(A.layer0, lw, lh, K, (m0x + lexf) + 0.5f, (m0y + lexf) + 0.5f);
        } else if (A.color_from == 2) {
            r = tap_layer_cubic<C>(A.layer1, lw, lh, K, (m1x + lexf) + 0.5f, (m1y + lexf) + 0.5f);
        } else {
            Texel<C> c0 = tap_layer_cubic<C>(A.layer0, lw, lh, K, (m0x + lexf) + 0.5f, (m0y + lexf) + 0.5f);
#pragma unroll
            for (int k = 0; k < C; ++k)
                asm volatile("" : "+v"(c0.c[k]));
            asm volatile("" : "+v"(m1x), "+v"(m1y));
            const Texel<C> c1 = tap_layer_cubic<C>(A.layer1, lw, lh, K, (m1x + lexf) + 0.5f, (m1y + lexf) + 0.5f);
#pragma unroll
            for (int k = 0; k < C; ++k)
                r.c[k] = c0.c[k] * (1 - color_fa) + c1.c[k] * color_fa;
        }
#pragma unroll
        for (int k = 0; k < C; ++k)
            acc[k] = acc[k] + r.c[k];
    }
}

// store_mean with the clamp: a cubic filter overshoots, so the mean of the canvases' samples is brought back to
// [0, 255] before the renderer's rounding (a NaN becomes 0: fmaxf); samples are not clamped one by one.  Layers are
// stored as they are: a matte may leave [0, 1], and what to do with that is the caller's decision.
template <int C, class Args> __device__ __forceinline__ void store_mean_clamped(const Args &A, int x, int y, const float (&acc)[NACC<C>], float n)
{
    if constexpr (C == CANVAS) {
        uint8_t *o = A.rgb + 3 * ((size_t)y * A.w + x);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[k] = (uint8_t)((double)fminf(fmaxf(__fdiv_rn(acc[k], n), 0.0f), 255.0f) + 0.5);
    } else {
        store_mean<C>(A, x, y, acc, n);
    }
}

} // namespace vm_chain

#endif
