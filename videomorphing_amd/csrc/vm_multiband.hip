// vm_multiband.hip -- the multiband render calls, for gfx950: the two plates the compositor's chain
// (kernel_render_halfway_image, Algorithm/render.cu:16-60; UI/RenderWidget.cpp:229-266; vm_chain.h, vm_chain_win.h) lands
// every output pixel on are blended band by band -- the multiresolution spline of Burt and Adelson (1983) -- instead of
// under one per-pixel weight.  Three kernel families, every expression in the order of tests/multiband_ref.py:
//
//   warp pass   k_mb_warp / k_mb_warp_win: the chain in its plain and its window form, with and without rates, with and
//               without a path; the tail forms c0 and c1 exactly as vm_warp.hip's tails do before they blend (the RGBA8
//               canvases at (map + ex) + 0.5f, the layers through vm_layer_tap.h at (map + lexf) + 0.5f) and writes them and
//               the colour weight A (color_fa, or k under a schedule) as float PLANES: level 0 of G0, G1 and M.
//   reduce      k_mb_reduce, one launch per level over the 2 C + 1 planes of G0, G1 and M together (blockIdx.z is the
//               plane): a workgroup stages the (2 TW + 3) x (2 TH + 3) source window of its TW x TH output tile in LDS once,
//               with the statement's fold (-1 -> 1, n -> n - 2) in the staging; a thread runs the row pass
//               (1 4 6 4 1) / 16 on the five rows of its output and then the column pass.
//   collapse    k_mb_base at the coarsest level (R = G0 (1 - m) + G1 m), then k_mb_collapse per level, coarsest first: a
//               workgroup stages the (TW / 2 + 2) x (TH / 2 + 2) coarse windows of G0[l+1], G1[l+1] and R[l+1] per channel;
//               the three expands share indices and parities; both Laplacian bands are formed on the fly (none is stored),
//               the mask is sharpened about 0.5 and clamped, the band blended and added to the expanded R.  At level 0 the
//               RGB8 instantiation clamps to [0, 255], rounds and writes bytes, the layer instantiations write interleaved
//               floats; above it R stays planar.
//
// Planes make every kernel after the warp pass a kernel over scalar images: the loads and stores of a wave are contiguous
// whatever the channel count, and the reduce needs no instantiation per channel count.  The x parity of a pixel differs
// from lane to lane and the y parity within a wave (two rows of 32), so the expand forms the even and the odd expression
// and selects: the selected bits are the statement's.
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_layer_tap.h"
#include "vm_multiband.h"

namespace {

using namespace vm_chain;

constexpr int CANVAS = VM_WARP_CANVAS;
constexpr int TW = 32, TH = 8;                      // a workgroup's tile: outputs of a reduce, fine pixels of a collapse
constexpr int SW = 2 * TW + 3, SH = 2 * TH + 3;     // the reduce's source window
constexpr int CW = TW / 2 + 2, CH = TH / 2 + 2;     // the collapse's coarse window
enum { OUT_PLANES = 0, OUT_TEXELS = 1, OUT_RGB8 = 2 };

// the statement's fold for the offsets the kernels use (+-2 of an index inside: two rounds suffice, n >= 2); a window
// cell no pixel of the image reads may lie further out and is clamped into the image
__device__ __forceinline__ int fold(int i, int n)
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        i = i < 0 ? -i : i;
        i = i >= n ? 2 * (n - 1) - i : i;
    }
    return min(max(i, 0), n - 1);
}

// ---------------------------------------------------------------------------
// the warp pass
struct VmMbWarp {
    int w, h, rs;
    float color_fa, geo_fa;
    const float2 *vf, *uf, *rates;
    const float *layer0, *layer1;
    int lw, lh;
    float lexf;
    const uchar4 *ext0, *ext1;
    int ex;
    float *g0, *g1, *mask;      // level 0: the planes of c0, of c1, and A
    size_t stride;
    int tiles_x, ntiles;
};

template <int C, bool RATES> __device__ __forceinline__ void plates_tail(const VmMbWarp &A, int x, int y, const Landing &L)
{
    const float m0x = L.px - L.v.x, m0y = L.py - L.v.y;
    const float m1x = L.px + L.v.x, m1y = L.py + L.v.y;
    const size_t at = (size_t)y * A.w + x;
    if constexpr (C == CANVAS) {
        const int cw = A.w + 2 * A.ex, ch = A.h + 2 * A.ex, ex = A.ex;
        const float3 c0 = tap_rgb(A.ext0, cw, ch, m0x + ex + 0.5f, m0y + ex + 0.5f);
        const float3 c1 = tap_rgb(A.ext1, cw, ch, m1x + ex + 0.5f, m1y + ex + 0.5f);
        A.g0[at] = c0.x; A.g0[A.stride + at] = c0.y; A.g0[2 * A.stride + at] = c0.z;
        A.g1[at] = c1.x; A.g1[A.stride + at] = c1.y; A.g1[2 * A.stride + at] = c1.z;
    } else {
        const Texel<C> c0 = tap_layer<C>(A.layer0, A.lw, A.lh, (m0x + A.lexf) + 0.5f, (m0y + A.lexf) + 0.5f);
        const Texel<C> c1 = tap_layer<C>(A.layer1, A.lw, A.lh, (m1x + A.lexf) + 0.5f, (m1y + A.lexf) + 0.5f);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            A.g0[k * A.stride + at] = c0.c[k];
            A.g1[k * A.stride + at] = c1.c[k];
        }
    }
    A.mask[at] = RATES ? L.k : A.color_fa;
}

// the plain form: one pixel per thread, every tap a global gather
template <int C, bool RATES> __global__ __launch_bounds__(256) void k_mb_warp(const VmMbWarp A)
{
    int x, y;
    Landing L;
    if (!chain_plain<RATES>(A.w, A.h, A.rs, A.geo_fa, A.vf, A.uf, A.rates, x, y, L))
        return;
    plates_tail<C, RATES>(A, x, y, L);
}

// the window form
template <bool HAS_U, int C, bool RATES> __global__ __launch_bounds__(RW * RH) void k_mb_warp_win(const VmMbWarp A)
{
    const int w = A.w, h = A.h, rs = A.rs, tiles_x = A.tiles_x, ntiles = A.ntiles;
    const float geo_fa = A.geo_fa;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf, *rates = A.rates;
#include "vm_chain_win.h"
    plates_tail<C, RATES>(A, x, y, L);
}

// ---------------------------------------------------------------------------
// reduce: plane blockIdx.z of a w x h level into its (w + 1) / 2 x (h + 1) / 2 one
__global__ __launch_bounds__(TW * TH) void k_mb_reduce(const float *__restrict__ src, float *__restrict__ dst, int w, int h,
                                                       size_t sstride, size_t dstride)
{
    __shared__ float win[SH * SW];
    const int mw = (w + 1) / 2, mh = (h + 1) / 2;
    src += blockIdx.z * sstride;
    dst += blockIdx.z * dstride;
    const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH, tid = threadIdx.y * TW + threadIdx.x;
    // window cell (wy, wx) is source sample (2 oy0 - 2 + wy, 2 ox0 - 2 + wx), folded into the level
    for (int i = tid; i < SH * SW; i += TW * TH) {
        const int wy = i / SW, wx = i - wy * SW;
        win[i] = src[(size_t)fold(2 * oy0 - 2 + wy, h) * w + fold(2 * ox0 - 2 + wx, w)];
    }
    __syncthreads();
    const int ox = ox0 + threadIdx.x, oy = oy0 + threadIdx.y;
    if (ox >= mw || oy >= mh)
        return;
    const float *p = win + 2 * threadIdx.y * SW + 2 * threadIdx.x;
    float row[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const float *q = p + r * SW;
        row[r] = (0.0625f * (q[0] + q[4]) + 0.25f * (q[1] + q[3])) + 0.375f * q[2];
    }
    dst[(size_t)oy * mw + ox] = (0.0625f * (row[0] + row[4]) + 0.25f * (row[1] + row[3])) + 0.375f * row[2];
}

// ---------------------------------------------------------------------------
// collapse
__device__ __forceinline__ float sharpened(float M, float sharp) { return fminf(fmaxf(0.5f + (M - 0.5f) * sharp, 0.0f), 1.0f); }

// the coarsest level: channel blockIdx.y of R = G0 (1 - m) + G1 m over the n cells of a plane
__global__ __launch_bounds__(256) void k_mb_base(const float *__restrict__ g, float *__restrict__ r, size_t n, size_t stride,
                                                 int channels, float sharp)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const int c = blockIdx.y;
    const float m = sharpened(g[2 * channels * stride + i], sharp);
    r[c * stride + i] = g[c * stride + i] * (1 - m) + g[(channels + c) * stride + i] * m;
}

// the statement's expand at one fine pixel from a coarse window: wn points at the cell of (j - 1, i - 1), i = x / 2, j = y / 2;
// along x first on the rows j - 1, j, j + 1, then along y
__device__ __forceinline__ float expand_at(const float *wn, bool odd_x, bool odd_y)
{
    float X[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float a = wn[j * CW], b = wn[j * CW + 1], c = wn[j * CW + 2];
        const float even = 0.125f * (a + c) + 0.75f * b, odd = 0.5f * (b + c);
        X[j] = odd_x ? odd : even;
    }
    const float even = 0.125f * (X[0] + X[2]) + 0.75f * X[1], odd = 0.5f * (X[1] + X[2]);
    return odd_y ? odd : even;
}

struct VmMbCollapse {
    int w, h, cw, ch;           // level l and level l + 1
    size_t stride, cstride;
    const float *g, *g1;        // the 2 C + 1 planes of level l; the planes of level l + 1 (G0 and G1 are read)
    const float *r1;            // R of level l + 1, C planes
    float *r;                   // OUT_PLANES: R of level l, C planes; OUT_TEXELS: (h, w, C) floats
    uint8_t *rgb;               // OUT_RGB8: (h, w, 3) bytes
    float sharp;
};

template <int C, int OUT> __global__ __launch_bounds__(TW * TH) void k_mb_collapse(const VmMbCollapse A)
{
    __shared__ float win[3 * C][CH * CW];       // G0[l + 1], G1[l + 1], R[l + 1], C channels each
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, tid = threadIdx.y * TW + threadIdx.x;
    // window cell (wy, wx) is coarse sample (y0 / 2 - 1 + wy, x0 / 2 - 1 + wx), folded into the coarse level
    for (int i = tid; i < 3 * C * CH * CW; i += TW * TH) {
        const int p = i / (CH * CW), cell = i - p * (CH * CW);
        const int wy = cell / CW, wx = cell - wy * CW;
        const float *src = p < 2 * C ? A.g1 + p * A.cstride : A.r1 + (p - 2 * C) * A.cstride;
        win[p][cell] = src[(size_t)fold(y0 / 2 - 1 + wy, A.ch) * A.cw + fold(x0 / 2 - 1 + wx, A.cw)];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= A.w || y >= A.h)
        return;
    const size_t at = (size_t)y * A.w + x;
    const float m = sharpened(A.g[2 * C * A.stride + at], A.sharp);
    const int cell = (threadIdx.y / 2) * CW + threadIdx.x / 2;
    const bool odd_x = x & 1, odd_y = y & 1;
    Texel<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float b0 = A.g[c * A.stride + at] - expand_at(win[c] + cell, odd_x, odd_y);
        const float b1 = A.g[(C + c) * A.stride + at] - expand_at(win[C + c] + cell, odd_x, odd_y);
        const float B = b0 * (1 - m) + b1 * m;
        r.c[c] = expand_at(win[2 * C + c] + cell, odd_x, odd_y) + B;
        // (a channel's value is opaque from here on: seeing the texel's store, the vectoriser otherwise forms the channels
        // side by side as vectors, and the four-channel kernel takes 92 VGPRs, five waves per SIMD where the LDS allows eight)
        asm volatile("" : "+v"(r.c[c]));
    }
    if constexpr (OUT == OUT_RGB8) {
        uint8_t *o = A.rgb + 3 * at;
#pragma unroll
        for (int c = 0; c < C; ++c)
            o[c] = (uint8_t)((double)fminf(fmaxf(r.c[c], 0.0f), 255.0f) + 0.5);
    } else if constexpr (OUT == OUT_TEXELS) {
        texel_store<C>(A.r, at, r);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c)
            A.r[c * A.stride + at] = r.c[c];
    }
}

dim3 tiles(int w, int h, int z) { return dim3((w + TW - 1) / TW, (h + TH - 1) / TH, z); }

template <bool RATES> void launch_warp(VmMbWarp &A, int channels, bool window, hipStream_t s)
{
    for_channels(channels, [&](auto c) {
        constexpr int C = decltype(c)::value;
        launch_form(window, A.w, A.h, A, k_mb_warp<C, RATES>, k_mb_warp_win<true, C, RATES>, k_mb_warp_win<false, C, RATES>, s);
    });
}

template <int C> void launch_collapse(const VmMbCollapse &A, int level, bool canvas, hipStream_t s)
{
    const dim3 g = tiles(A.w, A.h, 1), b(TW, TH);
    if (level)
        hipLaunchKernelGGL((k_mb_collapse<C, OUT_PLANES>), g, b, 0, s, A);
    else if (!canvas)
        hipLaunchKernelGGL((k_mb_collapse<C, OUT_TEXELS>), g, b, 0, s, A);
    else if constexpr (C == 3)
        hipLaunchKernelGGL((k_mb_collapse<3, OUT_RGB8>), g, b, 0, s, A);
}

} // namespace

void vm_launch_multiband(const VmMultiband &M, hipStream_t s)
{
    const bool canvas = M.channels < 1 || M.channels > 4;
    const int C = canvas ? 3 : M.channels, L = M.levels;
    const VmMbLayout Y = vm_mb_layout(M.w, M.h, C, L);
    // the warp pass: level 0 of G0, G1 and M
    VmMbWarp A{};
    A.w = M.w; A.h = M.h; A.rs = M.rs;
    A.color_fa = M.color_fa; A.geo_fa = M.geo_fa;
    A.vf = M.vf; A.uf = M.uf; A.rates = M.rates;
    A.layer0 = M.layer0; A.layer1 = M.layer1; A.lw = M.lw; A.lh = M.lh; A.lexf = M.lexf;
    A.ext0 = M.ext0; A.ext1 = M.ext1; A.ex = M.ex;
    A.stride = Y.stride[0];
    A.g0 = M.ws + Y.g[0]; A.g1 = A.g0 + C * Y.stride[0]; A.mask = A.g0 + 2 * C * Y.stride[0];
    const bool window = vm_render_window_form(M.rs, M.h);
    if (M.rates) {
        VmTransition T{};
        T.w = M.w; T.h = M.h; T.rs = M.rs;
        T.t = M.t; T.ease = M.ease;
        T.sched_geo = M.sched_geo; T.sched_color = M.sched_color; T.rates = M.rates;
        vm_launch_rates(T, s);
        launch_warp<true>(A, canvas ? CANVAS : C, window, s);
    } else {
        launch_warp<false>(A, canvas ? CANVAS : C, window, s);
    }
    // reduce: level l into level l + 1, the 2 C + 1 planes together
    for (int l = 0; l < L; ++l)
        hipLaunchKernelGGL(k_mb_reduce, tiles(Y.w[l + 1], Y.h[l + 1], 2 * C + 1), dim3(TW, TH), 0, s, M.ws + Y.g[l], M.ws + Y.g[l + 1],
                           Y.w[l], Y.h[l], Y.stride[l], Y.stride[l + 1]);
    // collapse: the coarsest level, then level by level down to the output
    const size_t n = (size_t)Y.w[L] * Y.h[L];
    hipLaunchKernelGGL(k_mb_base, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, s, M.ws + Y.g[L], M.ws + Y.r[L], n, Y.stride[L], C,
                       M.sharp[L]);
    for (int l = L - 1; l >= 0; --l) {
        VmMbCollapse K{};
        K.w = Y.w[l]; K.h = Y.h[l]; K.cw = Y.w[l + 1]; K.ch = Y.h[l + 1];
        K.stride = Y.stride[l]; K.cstride = Y.stride[l + 1];
        K.g = M.ws + Y.g[l]; K.g1 = M.ws + Y.g[l + 1]; K.r1 = M.ws + Y.r[l + 1];
        K.r = l ? M.ws + Y.r[l] : M.out;
        K.rgb = M.rgb;
        K.sharp = M.sharp[l];
        for_channels<false, false>(C, [&](auto c) { launch_collapse<decltype(c)::value>(K, l, canvas, s); });
    }
}
