// vm_tshutter.hip -- motion blur under a transition schedule for gfx950: the compositor's chain
// (kernel_render_halfway_image, Algorithm/render.cu:16-60; vm_chain.h, vm_chain_win.h) with per-texel rates
// walked at the N sample times of a shutter per output pixel.  One pre-pass and one launch per call,
// whatever N is, and no device memory that grows with N.
//
// In float32, without contraction, with ramp and tapr as vm_warp.hip states them (1 <= N <= 64):
//   K   = ramp(schedule_colour, t_color, ease)                             once per call: a dissolve is not motion
//   for s = 0 .. N - 1:
//     f   = ((float)s + 0.5f) / (float)N                                   correctly rounded division
//     t_s = t_open + (t_close - t_open) * f                                not clamped: ramp clamps per texel
//     G_s = ramp(schedule_geometry, t_s, ease)
//     (p, V)_s = the chain under G_s: g = tapr(G_s, p) anew at every p, the window where the centre's own G_s sends it
//     k_s = tapr(K, p_s)
//     c_s = the tail of the transition call: canvas or layer taps, blended by color_from with k_s
//     acc = acc + c_s                                                      acc starts at +0, in sample order
// and the pixel is (uint8)((double)(acc / (float)N) + 0.5) per channel for the canvases, acc / (float)N for layers.
//
// G_s is never stored.  The pre-pass (k_rates of vm_warp.hip, at t_color) leaves K in the .y of the frame's rate plane;
// the kernels hand the chain a Ramped (vm_ramp.h) in the place of its rate plane, and the chain's rate_at / rate_texel
// ramp the geometry schedule at t_s where they read it: every cell the window form stages (one division per staged cell
// and sample), the four texels of a tap outside the window, every rate texel of the plain form.
//
// The window form restages (G, K) at every sample -- G_s has changed even where the window has not moved -- after a
// barrier from the second sample on (every tap of the sample before has been served; a thread without a pixel stays in
// the loop for it), and v and u only where the window's origin has moved (restage<true> of vm_shutter_tail.h).
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_ramp.h"
#include "vm_shutter_tail.h"
#include "vm_tshutter.h"

namespace {

using namespace vm_chain;

// the plain form: one pixel per thread, every tap a global gather, every rate texel ramped where it is read
template <int C> __global__ __launch_bounds__(256) void k_tblur(const VmTShutter A)
{
    const float n = (float)A.samples;
    float acc[NACC<C>] = {};
    int x = 0, y = 0;
    for (int s = 0; s < A.samples; ++s) {
        const Ramped rates{A.sched_geo, A.rates, sample_time<false>(A.t_open, A.t_close, s, n), A.ease};
        Landing L;
        if (!chain_plain<true>(A.w, A.h, A.rs, 0.0f, A.vf, A.uf, rates, x, y, L))
            return;
        add_sample<C>(A, L, L.k, acc);
    }
    store_mean<C>(A, x, y, acc, n);
}

// the window form.  The chain's statements stand in the sample loop, as in k_shutter_win: a thread without a pixel goes
// on to the next sample's barriers, only the workgroup past the last tile leaves, and the one store stands behind the
// last sample inside the loop.
#define VM_CHAIN_WIN_NO_PIXEL continue
#define VM_CHAIN_WIN_STAGE(ox, oy) restage<true>(s, ox, oy, at_x, at_y, moved)
#define VM_CHAIN_WIN_STAGE_FIELD moved
template <bool HAS_U, int C> __global__ __launch_bounds__(RW * RH) void k_tblur_win(const VmTShutter A)
{
    constexpr bool RATES = true;
    const int rs = A.rs, ntiles = A.ntiles;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf;
    const float geo_fa = 0.0f;          // (the chain's uniform rate: under RATES every round takes its own g)
    float acc[NACC<C>] = {};
    int at_x = 0, at_y = 0;             // where the staged window is (read from the second sample on: restage())
    bool moved = true;
    for (int s = 0; s < A.samples; ++s) {
        const int w = per_sample(A.w), h = per_sample(A.h), tiles_x = per_sample(A.tiles_x);
        const float n = (float)per_sample(A.samples);
        const Ramped rates{A.sched_geo, A.rates, sample_time<false>(per_sample(A.t_open), A.t_close, s, n), A.ease};
#include "vm_chain_win.h"
        add_sample<C>(A, L, L.k, acc);
        if (s == A.samples - 1)
            store_mean<C>(A, x, y, acc, n);
    }
}
#undef VM_CHAIN_WIN_NO_PIXEL
#undef VM_CHAIN_WIN_STAGE
#undef VM_CHAIN_WIN_STAGE_FIELD

} // namespace

void vm_launch_tshutter(const VmTShutter &S, hipStream_t s)
{
    VmTShutter A = S;
    launch_colour_rates(A, s);
    for_channels(A.channels, [&](auto c) {
        constexpr int C = decltype(c)::value;
        launch_form(vm_render_window_form(A.rs, A.h), A.w, A.h, A, k_tblur<C>, k_tblur_win<true, C>, k_tblur_win<false, C>, s);
    });
}
