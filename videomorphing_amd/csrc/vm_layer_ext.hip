// vm_layer_ext.hip -- Poisson boundary extension of float layers on the device (gfx950).
//
// What: CPoissonExt::prepare + poissonExtend, Algorithm/PoissonExt.cpp:49-362, for one side of a frame's float layers of
// 1..4 interleaved channels: the float counterpart of vm_poisson.hip's k_canvas, k_classify, k_fill, k_setup and k_paste.
// The canvas is (ch, cw, C) float32 with the tight layer at (ex, ex); a byte plane `valid` says where a cell holds a value
// (the RGB path's magenta marker has no float counterpart).  A layer has no alpha, so the type map is geometric -- the map
// k_classify gives for a canvas built by k_canvas: 2 outside the image, 1 on the image's outermost ring, else 0
// (PoissonExt.cpp:59-101).  The fill (:104-137) follows the halfway field into the other side's tight layer with k_fill's
// expressions in k_fill's order and keeps the bilinear value unrounded; the right-hand side and the initial guess
// (:146-270) are k_setup's statement on floats, zero on holes; the paste (:333-346) takes the solution as it is.
//
// How: the system is the RGB path's and is solved by the same batched multigrid-preconditioned CG (vm_mgb.hip), three
// channels per 12-byte vector entry: a 4-channel layer travels as two groups, unused lanes are zero (and stay zero: the
// solver's step lengths are per lane).
#include "vm_internal.h"
#include "vm_layer_ext.h"
#include "vm_mgb.h"
#include <type_traits>

namespace {

inline dim3 grid2(int w, int h) { return dim3((w + 63) / 64, (h + 3) / 4); }
const dim3 B2(64, 4);

template <int C> __global__ __launch_bounds__(256) void k_lx_canvas(float *ext, uint8_t *valid, const float *__restrict__ tight,
                                                                    int w, int h, int ex)
{
    const int cw = w + 2 * ex, ch = h + 2 * ex;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cw || y >= ch)
        return;
    const int fx = x - ex, fy = y - ex;
    const bool in = fx >= 0 && fx < w && fy >= 0 && fy < h;
    const size_t ii = (size_t)y * cw + x;
#pragma unroll
    for (int k = 0; k < C; ++k)
        ext[ii * C + k] = in ? tight[((size_t)fy * w + fx) * C + k] : 0.0f;
    valid[ii] = in ? 1 : 0;
}

// classification, PoissonExt.cpp:59-101, of a canvas whose alpha is 0 on the image and > 0 around it
__global__ __launch_bounds__(256) void k_lx_type(uint8_t *type, int w, int h, int ex)
{
    const int cw = w + 2 * ex, ch = h + 2 * ex;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cw || y >= ch)
        return;
    const int fx = x - ex, fy = y - ex;
    uint8_t t = 0;
    if (fx < 0 || fx >= w || fy < 0 || fy >= h)
        t = 2;
    else if (ex > 0 && (fx == 0 || fx == w - 1 || fy == 0 || fy == h - 1))
        t = 1;
    type[(size_t)y * cw + x] = t;
}

// BilineaGetColor_clamp<Vec2f,Vec2f>, PoissonExt.cpp:367-397
__device__ __forceinline__ float2 bil_v(const float2 *__restrict__ v, int w, int h, int rs, float px, float py)
{
    const int x0 = (int)floorf(px), y0 = (int)floorf(py);
    const int x1 = (int)ceilf(px), y1 = (int)ceilf(py);
    const float a = px - x0, b = py - y0;
    const int cx0 = min(max(x0, 0), w - 1), cx1 = min(max(x1, 0), w - 1);
    const int cy0 = min(max(y0, 0), h - 1), cy1 = min(max(y1, 0), h - 1);
    const float2 v00 = v[cy0 * rs + cx0], v01 = v[cy1 * rs + cx0];
    const float2 v10 = v[cy0 * rs + cx1], v11 = v[cy1 * rs + cx1];
    float2 r;
    r.x = v00.x * (1 - a) * (1 - b) + v01.x * (1 - a) * b + v10.x * a * (1 - b) + v11.x * a * b;
    r.y = v00.y * (1 - a) * (1 - b) + v01.y * (1 - a) * b + v10.y * a * (1 - b) + v11.y * a * b;
    return r;
}

// outside-cell fill, PoissonExt.cpp:104-137
template <int C> __global__ __launch_bounds__(256) void k_lx_fill(float *ext, uint8_t *valid, const uint8_t *__restrict__ type,
                                                                  const float *__restrict__ other,
                                                                  const float2 *__restrict__ vf, int w, int h, int rs, int ex,
                                                                  int sign)
{
    const int cw = w + 2 * ex, ch = h + 2 * ex;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cw || y >= ch)
        return;
    const size_t ii = (size_t)y * cw + x;
    if (type[ii] != 2)
        return;
    const float sg = (float)sign;
    float qx = (float)(x - ex), qy = (float)(y - ex);
    float px = qx, py = qy;
    float2 v = bil_v(vf, w, h, rs, px, py);
    const float al = 0.8f;
    for (int i = 0; i < 20; ++i) {
        px = qx + v.x * sg;
        py = qy + v.y * sg;
        float2 t = bil_v(vf, w, h, rs, px, py);
        v.x = al * t.x + (1 - al) * v.x;
        v.y = al * t.y + (1 - al) * v.y;
    }
    qx = px + v.x * sg;
    qy = py + v.y * sg;
    float o[C];
#pragma unroll
    for (int k = 0; k < C; ++k)
        o[k] = 0.0f;
    uint8_t ok = 0;
    if (qx >= 0 && qy >= 0 && qx < w && qy < h) {
        const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
        const int x1 = (int)ceilf(qx), y1 = (int)ceilf(qy);
        const float a = qx - x0, b = qy - y0;
        const int cx0 = min(max(x0, 0), w - 1), cx1 = min(max(x1, 0), w - 1);
        const int cy0 = min(max(y0, 0), h - 1), cy1 = min(max(y1, 0), h - 1);
        const float *c00 = other + ((size_t)cy0 * w + cx0) * C, *c01 = other + ((size_t)cy1 * w + cx0) * C;
        const float *c10 = other + ((size_t)cy0 * w + cx1) * C, *c11 = other + ((size_t)cy1 * w + cx1) * C;
#pragma unroll
        for (int k = 0; k < C; ++k)
            o[k] = c00[k] * (1 - a) * (1 - b) + c01[k] * (1 - a) * b + c10[k] * a * (1 - b) + c11[k] * a * b;
        ok = 1;
    }
#pragma unroll
    for (int k = 0; k < C; ++k)
        ext[ii * C + k] = o[k];
    valid[ii] = ok;
}

// the n channels from c0 of cell i, the other lanes zero
__device__ __forceinline__ float3 lanes(const float *__restrict__ ext, size_t i, int C, int c0, int n)
{
    const float *p = ext + i * C + c0;
    return make_float3(p[0], n > 1 ? p[1] : 0.0f, n > 2 ? p[2] : 0.0f);
}

// gx / gy of PoissonExt.cpp:146-183: value(a) - value(b) when both are outside cells that hold a value, else 0
__device__ __forceinline__ float3 grad(const float *__restrict__ ext, const uint8_t *__restrict__ valid,
                                       const uint8_t *__restrict__ type, size_t a, size_t b, int C, int c0, int n)
{
    if (type[a] <= 1 || type[b] <= 1)
        return make_float3(0, 0, 0);
    if (valid[a] == 0 || valid[b] == 0)
        return make_float3(0, 0, 0);
    const float3 ca = lanes(ext, a, C, c0, n), cb = lanes(ext, b, C, c0, n);
    return make_float3(ca.x - cb.x, ca.y - cb.y, ca.z - cb.z);
}

// right-hand side, PoissonExt.cpp:214-270, and the initial guess
__global__ __launch_bounds__(256) void k_lx_setup(const float *__restrict__ ext, const uint8_t *__restrict__ valid,
                                                  const uint8_t *__restrict__ type, VmV3 *B, VmV3 *X, int *nz, int cw, int ch,
                                                  int C, int c0, int n)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cw || y >= ch)
        return;
    const size_t ii = (size_t)y * cw + x;
    const uint8_t t = type[ii];
    float3 b = make_float3(0, 0, 0);
    if (t == 1) {
        const float3 c = lanes(ext, ii, C, c0, n);
        b.x += c.x; b.y += c.y; b.z += c.z;
    }
    if (t > 0) {
        if (y - 1 >= 0 && type[ii - cw] > 0) { float3 g = grad(ext, valid, type, ii, ii - cw, C, c0, n); b.x += g.x; b.y += g.y; b.z += g.z; }
        if (x - 1 >= 0 && type[ii - 1] > 0) { float3 g = grad(ext, valid, type, ii, ii - 1, C, c0, n); b.x += g.x; b.y += g.y; b.z += g.z; }
        if (x + 1 < cw && type[ii + 1] > 0) { float3 g = grad(ext, valid, type, ii + 1, ii, C, c0, n); b.x -= g.x; b.y -= g.y; b.z -= g.z; }
        if (y + 1 < ch && type[ii + cw] > 0) { float3 g = grad(ext, valid, type, ii + cw, ii, C, c0, n); b.x -= g.x; b.y -= g.y; b.z -= g.z; }
    }
    B[ii] = VmV3{b.x, b.y, b.z};
    if (b.x != 0.0f || b.y != 0.0f || b.z != 0.0f)      // (a NaN raises it too: the solver's own check then refuses it)
        *nz = 1;
    // initial guess: the value already there (ring and filled cells), zero on holes
    float3 x0 = make_float3(0, 0, 0);
    if (t > 0 && valid[ii] != 0)
        x0 = lanes(ext, ii, C, c0, n);
    X[ii] = VmV3{x0.x, x0.y, x0.z};
}

// paste, PoissonExt.cpp:333-346, unclamped
__global__ __launch_bounds__(256) void k_lx_paste(float *ext, uint8_t *valid, const uint8_t *__restrict__ type,
                                                  const VmV3 *__restrict__ X, int cw, int ch, int C, int c0, int n, int set_valid)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cw || y >= ch)
        return;
    const size_t ii = (size_t)y * cw + x;
    if (type[ii] == 0)
        return;
    const VmV3 v = X[ii];
    float *p = ext + ii * C + c0;
    p[0] = v.x;
    if (n > 1) p[1] = v.y;
    if (n > 2) p[2] = v.z;
    if (set_valid)
        valid[ii] = 1;
}

// f(integral_constant<int, C>) for the C in 1..4 the frame's layers have
template <class F> void for_layer_channels(int C, F f)
{
    switch (C) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    }
}

} // namespace

void vm_layer_ext_launch_canvas(float *ext, uint8_t *valid, const float *tight, int C, int w, int h, int ex, hipStream_t s)
{
    for_layer_channels(C, [&](auto c) {
        hipLaunchKernelGGL(k_lx_canvas<decltype(c)::value>, grid2(w + 2 * ex, h + 2 * ex), B2, 0, s, ext, valid, tight, w, h, ex);
    });
}

void vm_layer_ext_launch_type(uint8_t *type, int w, int h, int ex, hipStream_t s)
{
    hipLaunchKernelGGL(k_lx_type, grid2(w + 2 * ex, h + 2 * ex), B2, 0, s, type, w, h, ex);
}

void vm_layer_ext_launch_fill(float *ext, uint8_t *valid, const uint8_t *type, const float *other, const float2 *v, int C, int w,
                              int h, int rs, int ex, int sign, hipStream_t s)
{
    for_layer_channels(C, [&](auto c) {
        hipLaunchKernelGGL(k_lx_fill<decltype(c)::value>, grid2(w + 2 * ex, h + 2 * ex), B2, 0, s, ext, valid, type, other, v, w, h,
                           rs, ex, sign);
    });
}

void vm_layer_ext_launch_setup(const float *ext, const uint8_t *valid, const uint8_t *type, VmV3 *B, VmV3 *X, int *nz, int cw,
                               int ch, int C, int c0, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_lx_setup, grid2(cw, ch), B2, 0, s, ext, valid, type, B, X, nz, cw, ch, C, c0, n);
}

void vm_layer_ext_launch_paste(float *ext, uint8_t *valid, const uint8_t *type, const VmV3 *X, int cw, int ch, int C, int c0,
                               int n, int set_valid, hipStream_t s)
{
    hipLaunchKernelGGL(k_lx_paste, grid2(cw, ch), B2, 0, s, ext, valid, type, X, cw, ch, C, c0, n, set_valid);
}
