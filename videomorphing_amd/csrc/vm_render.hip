// vm_render.hip -- compositor and result-delivery kernels for gfx950.
//
// k_render / k_render_win: kernel_render_halfway_image, Algorithm/render.cu:16-60.  The
//   reference samples float4 textures that RenderStage2 re-uploads every frame
//   (UI/RenderWidget.cpp:229-266); here the Poisson-extended canvases stay
//   resident as RGBA8 (uchar -> float is exact, so the taps see the same
//   values) and v/u as pitched float2: 8 B + 8 B + 3 B of compulsory traffic
//   per pixel plus gathered canvas taps served by L2.  The fixed-point chain
//   itself is stated in vm_chain.h, which vm_warp.hip shares: k_render_win, the
//   product path, walks the window form (vm_chain_win.h: the taps of v / u
//   served from an LDS window), k_render chain_plain (VM_RENDER=plain, and
//   fields of 4 GiB and more); this unit adds the RGB8 tail and the switch
//   between the two forms.
// k_upscale: CMatchingThread::update_result + Resize,
//   Algorithm/MatchingThread.cpp:22-136.
#include "vm_internal.h"
#include "vm_chain.h"
#include "vm_chain_launch.h"    // (and vm_warp.h for vm_render_window_form: vm_internal.h is part of the sweep profile's source fingerprint)
#include <cstdlib>
#include <cstring>

namespace {

using namespace vm_chain;

__global__ __launch_bounds__(256) void k_render(uint8_t *__restrict__ out, int out_pitch, int w,
                                                int h, int rs, int ex, float color_fa,
                                                float geo_fa, int color_from,
                                                const uchar4 *__restrict__ ext0,
                                                const uchar4 *__restrict__ ext1,
                                                const float2 *__restrict__ vf,
                                                const float2 *__restrict__ uf)
{
    int x, y;
    Landing L;
    if (!chain_plain<false>(w, h, rs, geo_fa, vf, uf, nullptr, x, y, L))
        return;
    const int cw = w + 2 * ex, ch = h + 2 * ex;
    const float3 c0 = tap_rgb(ext0, cw, ch, L.px - L.v.x + ex + 0.5f, L.py - L.v.y + ex + 0.5f);
    const float3 c1 = tap_rgb(ext1, cw, ch, L.px + L.v.x + ex + 0.5f, L.py + L.v.y + ex + 0.5f);
    rgb8_store(out + (size_t)y * out_pitch + 3 * x, c0, c1, color_from, color_fa);
}

template <bool HAS_U>
__global__ __launch_bounds__(RW * RH) void k_render_win(uint8_t *__restrict__ out, int out_pitch, int w, int h, int rs, int ex,
                                                    float color_fa, float geo_fa, int color_from,
                                                    const uchar4 *__restrict__ ext0, const uchar4 *__restrict__ ext1,
                                                    const float2 *__restrict__ vf, const float2 *__restrict__ uf, int tiles_x,
                                                    int ntiles, bool lean_canvas)
{
    constexpr bool RATES = false;
    const float2 *rates = nullptr;
#include "vm_chain_win.h"
    const int cw = w + 2 * ex, ch = h + 2 * ex;
    const float px = L.px, py = L.py; const float2 v = L.v;
    float3 c0, c1;
    if (lean_canvas) {      // 32-bit texel offsets, 24-bit rows (vm_launch_render)
        c0 = tap_rgb_lean(ext0, (float)cw, (float)ch, cw - 1, ch - 1, (uint32_t)cw, px - v.x + ex + 0.5f, py - v.y + ex + 0.5f);
        c1 = tap_rgb_lean(ext1, (float)cw, (float)ch, cw - 1, ch - 1, (uint32_t)cw, px + v.x + ex + 0.5f, py + v.y + ex + 0.5f);
    } else {
        c0 = tap_rgb(ext0, cw, ch, px - v.x + ex + 0.5f, py - v.y + ex + 0.5f);
        c1 = tap_rgb(ext1, cw, ch, px + v.x + ex + 0.5f, py + v.y + ex + 0.5f);
    }
    rgb8_store(out + (size_t)y * out_pitch + 3 * x, c0, c1, color_from, color_fa);
}

// BiLinear of MatchingThread.cpp:103-136 on the level's v scaled by (rx, ry)
__global__ __launch_bounds__(256) void k_upscale(float2 *__restrict__ dst, int w0, int h0,
                                                 int dpitch, const float2 *__restrict__ v, int w,
                                                 int h, int rs)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w0 || y >= h0)
        return;
    const float rx = (float)w0 / (float)w, ry = (float)h0 / (float)h;
    if (w == w0 && h == h0) {
        float2 s = v[y * rs + x];
        dst[(size_t)y * dpitch + x] = s; // ratio 1: copied unscaled (MatchingThread.cpp:42,55-58)
        return;
    }
    const float fy = (float)((y + 0.5) / h0 * h - 0.5);
    const float fx = (float)((x + 0.5) / w0 * w - 0.5);
    int xi[2] = {(int)floorf(fx), (int)ceilf(fx)};
    int yi[2] = {(int)floorf(fy), (int)ceilf(fy)};
    const float uu = fx - xi[0], vv = fy - yi[0];
    float2 val[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int tx = min(max(xi[i], 0), w - 1), ty = min(max(yi[j], 0), h - 1);
            float2 s = v[ty * rs + tx];
            val[i][j] = make_float2(s.x * rx, s.y * ry);
        }
    float2 r;
    r.x = val[0][0].x * (1 - uu) * (1 - vv) + val[0][1].x * (1 - uu) * vv +
          val[1][0].x * uu * (1 - vv) + val[1][1].x * uu * vv;
    r.y = val[0][0].y * (1 - uu) * (1 - vv) + val[0][1].y * (1 - uu) * vv +
          val[1][0].y * uu * (1 - vv) + val[1][1].y * uu * vv;
    dst[(size_t)y * dpitch + x] = r;
}

// the frames the temporal pyramid skipped: _vector[beg] * (1 - fa) + _vector[end] * fa
// (MatchingThread.cpp:62-78; a cv::Mat expression = addWeighted in float: two products, one sum)
__global__ __launch_bounds__(256) void k_blend_v(float2 *__restrict__ dst, int dpitch, const float2 *__restrict__ a,
                                                 const float2 *__restrict__ b, int spitch, int w0, int h0, float alpha,
                                                 float beta)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w0 || y >= h0)
        return;
    const float2 p = a[(size_t)y * spitch + x], q = b[(size_t)y * spitch + x];
    float2 r;
    r.x = p.x * alpha + q.x * beta;
    r.y = p.y * alpha + q.y * beta;
    dst[(size_t)y * dpitch + x] = r;
}

} // namespace

void vm_launch_blend_v(float2 *dst, int dpitch, const float2 *a, const float2 *b, int spitch, int w0, int h0,
                       float alpha, float beta, hipStream_t s)
{
    const Grid G = plain_grid(w0, h0);
    hipLaunchKernelGGL(k_blend_v, G.g, G.b, 0, s, dst, dpitch, a, b, spitch, w0, h0, alpha, beta);
}

void vm_launch_upscale(float2 *dst, int w0, int h0, int dpitch, const float2 *v, int w, int h,
                       int rs, hipStream_t s)
{
    const Grid G = plain_grid(w0, h0);
    hipLaunchKernelGGL(k_upscale, G.g, G.b, 0, s, dst, w0, h0, dpitch, v, w, h, rs);
}

// a kernel that only takes time: one wave reading the constant 100 MHz counter until `ticks` have passed
__global__ __launch_bounds__(64) void k_spin(unsigned long long ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks)
        __builtin_amdgcn_s_sleep(8);
}

void vm_launch_spin(unsigned long long ticks, int workgroups, hipStream_t s) { hipLaunchKernelGGL(k_spin, dim3(workgroups), dim3(64), 0, s, ticks); }

// (vm_warp.h) the window form addresses the field's texels by 32-bit byte offsets and multiplies rows in 24 bits
bool vm_render_window_form(int rs, int h)
{
    static const char *mode = getenv("VM_RENDER");
    static const bool plain = mode && !strcmp(mode, "plain");
    const bool small = (uint64_t)rs * (uint64_t)h * 8ull < (1ull << 32) && rs < (1 << 24) && h < (1 << 24);
    return small && !plain;
}

void vm_launch_render(uint8_t *out, int out_pitch, int w, int h, int rs, int ex, float color_fa,
                      float geo_fa, int color_from, const uchar4 *ext0, const uchar4 *ext1,
                      const float2 *v, const float2 *u, hipStream_t s)
{
    if (!vm_render_window_form(rs, h)) {
        const Grid G = plain_grid(w, h);
        hipLaunchKernelGGL(k_render, G.g, G.b, 0, s, out, out_pitch, w, h, rs, ex, color_fa, geo_fa, color_from, ext0, ext1, v, u);
        return;
    }
    struct { int tiles_x, ntiles; } T;
    const Grid G = window_grid(T, w, h);
    const uint64_t cw = (uint64_t)w + 2 * (uint64_t)ex, ch = (uint64_t)h + 2 * (uint64_t)ex;
    const bool lean_canvas = cw * ch * 4ull < (1ull << 32) && cw < (1u << 24) && ch < (1u << 24);   // 32-bit texel offsets, 24-bit rows
    if (u)
        hipLaunchKernelGGL(k_render_win<true>, G.g, G.b, 0, s, out, out_pitch, w, h, rs, ex, color_fa, geo_fa, color_from, ext0,
                           ext1, v, u, T.tiles_x, T.ntiles, lean_canvas);
    else
        hipLaunchKernelGGL(k_render_win<false>, G.g, G.b, 0, s, out, out_pitch, w, h, rs, ex, color_fa, geo_fa, color_from, ext0,
                           ext1, v, u, T.tiles_x, T.ntiles, lean_canvas);
}
