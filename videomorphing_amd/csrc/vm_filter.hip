// vm_filter.hip -- the viewport calls with a cubic filter on their last taps, for gfx950: the kernels of
// vm_viewport.hip -- the compositor's chain (kernel_render_halfway_image, Algorithm/render.cu:16-60; vm_chain.h,
// vm_chain_win.h) from the nx x ny sub-sample points of every pixel of an output grid laid freely over the halfway domain,
// the samples' colours summed in registers and stored once -- with add_sample_cubic (vm_filter_tap.h) in the place of
// add_sample: a canvas or a layer is read through 4 x 4 texels under Catmull-Rom, Mitchell or the cubic B-spline, whose
// coefficients are the launch's arguments.  q, the chain, (map0, map1)_s = (p - V, p + V), the blend, the sum in sample
// order and acc / (float)N are vm_viewport.hip's, statement by statement; the RGB8 result is clamped to [0, 255] before
// the renderer's rounding, layers are stored unclamped.  The chain's own 21 taps stay bilinear: it taps a smooth vector
// field, and its bits are the reference's.  The bilinear filter has no kernel here: it is vm_launch_viewport.
//
// The forms are vm_viewport.hip's: the window form for steps up to 1, staged by sample 0 alone, the plain form for any step.
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_filter.h"
#include "vm_filter_tap.h"
#include "vm_viewport_win.h"        // sample_q, cell_at, Out, and the hooks of the window form

namespace {

using namespace vm_chain;

// the plain form: one output pixel per thread, every tap a global gather; any step
template <int C> __global__ __launch_bounds__(256) void k_fview(const VmFiltered A)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.out_w || y >= A.out_h)
        return;
    float acc[NACC<C>] = {};
    for (int j = 0; j < A.ny; ++j)
        for (int i = 0; i < A.nx; ++i) {
            const float nx = (float)(C == CANVAS ? A.nx : per_sample(A.nx)), ny = (float)(C == CANVAS ? A.ny : per_sample(A.ny));
            Landing L;
            chain_plain_from<false>(A.w, A.h, A.rs, A.geo_fa, A.vf, A.uf, nullptr, sample_q(A.x0, A.step_x, x, i, nx),
                                    sample_q(A.y0, A.step_y, y, j, ny), L);
            add_sample_cubic<C>(A, L, per_sample(A.color_fa), acc);
        }
    store_mean_clamped<C>(Out{A.out_w, A.rgb, A.out}, x, y, acc, (float)(A.nx * A.ny));
}

// the window form: k_viewport_win's loop (the window belongs to the tile, sample 0 stages it, the one store stands behind
// the last sample inside the loop) with the cubic tail
#define VM_CHAIN_WIN_STAGE(ox, oy) (s == 0)
template <bool HAS_U, int C> __global__ __launch_bounds__(RW * RH) void k_fview_win(const VmFiltered A)
{
    constexpr bool RATES = false;
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
        add_sample_cubic<C>(A, L, per_sample(A.color_fa), acc);
        if (s == samples - 1)
            store_mean_clamped<C>(Out{A.out_w, A.rgb, A.out}, x, y, acc, (float)per_sample(samples));
        if (++si == A.nx) {
            si = 0;
            ++sj;
        }
    }
}
#undef VM_CHAIN_WIN_STAGE
#include "vm_viewport_win.h"        // (the hooks leave)

} // namespace

void vm_launch_filtered(const VmFiltered &V, hipStream_t s)
{
    VmFiltered A = V;
    for_channels(A.channels, [&](auto c) {
        constexpr int C = decltype(c)::value;
        launch_form(viewport_window_form(A), A.out_w, A.out_h, A, k_fview<C>, k_fview_win<true, C>, k_fview_win<false, C>, s);
    });
}
