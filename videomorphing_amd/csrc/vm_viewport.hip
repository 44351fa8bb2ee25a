// vm_viewport.hip -- any viewport of the morph at any size, supersampled, for gfx950: the compositor's chain
// (kernel_render_halfway_image, Algorithm/render.cu:16-60; vm_chain.h, vm_chain_win.h) started from the nx x ny sub-sample
// points of every pixel of an output grid laid freely over the halfway domain, the samples' colours summed in registers
// and stored once.  One launch per call, whatever N = nx * ny is.
//
// In float32, without contraction, for output pixel (X, Y) and s = j * nx + i = 0 .. N - 1 (1 <= N <= 64):
//   fx = ((float)i + 0.5f) / (float)nx,  fy = ((float)j + 0.5f) / (float)ny        correctly rounded divisions
//   qx = (x0 + ((float)X + fx) * step_x) - 0.5f,  qy = (y0 + ((float)Y + fy) * step_y) - 0.5f
//   (map0, map1)_s = the chain from q = (qx, qy) at the call's geo_fa
//   c_s = the tail of the uniform call on them: the canvas taps of vm_render.hip (+ ex, then + 0.5f, tap_rgb's weights) or
//         the layer taps of vm_warp.hip, blended by color_from with the call's color_fa
//   acc = acc + c_s                                                        acc starts at +0, in sample order
// and the pixel is (uint8)((double)(acc / (float)N) + 0.5) per channel for the canvases, acc / (float)N for layers.  With
// {0, 0, 1, 1, w, h, 1, 1} q is the pixel itself and that is the uniform call's result, bit for bit.
//
// The window form runs for steps up to 1: a tile of RW x RH output pixels then covers at most (RW + 1) x (RH + 1) field
// cells, which the window of vm_chain_win.h holds with its margin as it holds a tile of the field.  The window is placed
// from the field cell nearest the tile's centre and staged by the first sample alone: every sample of every pixel of the
// tile taps it, and no barrier follows the first.  A tap outside the window takes the global path, so the placement
// cannot change a bit.  Larger steps (a proxy, a thumbnail) run the plain form.
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_shutter_tail.h"
#include "vm_viewport.h"
#include "vm_viewport_win.h"        // sample_q, cell_at, Out, next_sub, and the hooks of the window form

namespace {

using namespace vm_chain;

// the plain form: one output pixel per thread, every tap a global gather; any step
template <int C> __global__ __launch_bounds__(256) void k_viewport(const VmViewport A)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.out_w || y >= A.out_h)
        return;
    float acc[NACC<C>] = {};
    for (int j = 0; j < A.ny; ++j)
        for (int i = 0; i < A.nx; ++i) {
            // (the layer tails: not held in vector registers across the chain -- their taps have a grid of their own to hold)
            const float nx = (float)(C == CANVAS ? A.nx : per_sample(A.nx)), ny = (float)(C == CANVAS ? A.ny : per_sample(A.ny));
            Landing L;
            chain_plain_from<false>(A.w, A.h, A.rs, A.geo_fa, A.vf, A.uf, nullptr, sample_q(A.x0, A.step_x, x, i, nx),
                                    sample_q(A.y0, A.step_y, y, j, ny), L);
            add_sample<C>(A, L, per_sample(A.color_fa), acc);
        }
    store_mean<C>(Out{A.out_w, A.rgb, A.out}, x, y, acc, (float)(A.nx * A.ny));
}

// the window form.  The chain's statements stand in the sample loop, as in vm_shutter.hip, but the window belongs to the
// tile, not to the sample: sample 0 stages it, a thread without a pixel leaves behind that one barrier, and the samples
// after it tap what is there.  x, y, tiles_x and ntiles count output pixels and tiles; (x, y) belong to the chain's
// statements, so the one store stands behind the last sample inside the loop.
#define VM_CHAIN_WIN_STAGE(ox, oy) (s == 0)
template <bool HAS_U, int C> __global__ __launch_bounds__(RW * RH) void k_viewport_win(const VmViewport A)
{
    constexpr bool RATES = false;       // (a viewport under a transition schedule or over a shutter is vm_vshutter.hip)
    const float2 *rates = nullptr;
    const int rs = A.rs, ntiles = A.ntiles;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf;
    const int samples = A.nx * A.ny;
    float acc[NACC<C>] = {};
    int si = 0, sj = 0;                 // sample s = sj * nx + si
    for (int s = 0; s < samples; ++s) {
        const int w = per_sample(A.w), h = per_sample(A.h), tiles_x = per_sample(A.tiles_x);
        const float geo_fa = per_sample(A.geo_fa);
#include "vm_chain_win.h"
        add_sample<C>(A, L, per_sample(A.color_fa), acc);
        if (s == samples - 1)
            store_mean<C>(Out{A.out_w, A.rgb, A.out}, x, y, acc, (float)per_sample(samples));
        if (++si == A.nx) {     // (not next_sub of vm_viewport_win.h: behind a function call all ten window kernels move)
            si = 0;
            ++sj;
        }
    }
}
#undef VM_CHAIN_WIN_STAGE
#include "vm_viewport_win.h"        // (the hooks leave)

} // namespace

void vm_launch_viewport(const VmViewport &V, hipStream_t s)
{
    VmViewport A = V;
    for_channels(A.channels, [&](auto c) {
        constexpr int C = decltype(c)::value;
        launch_form(viewport_window_form(A), A.out_w, A.out_h, A, k_viewport<C>, k_viewport_win<true, C>, k_viewport_win<false, C>, s);
    });
}
