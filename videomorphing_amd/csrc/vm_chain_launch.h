// vm_chain_launch.h -- how the units that walk the compositor's chain (vm_chain.h) launch their kernels, stated once for
// vm_render.hip, vm_warp.hip, vm_shutter.hip, vm_tshutter.hip, vm_viewport.hip, vm_vshutter.hip, vm_carry.hip and vm_multiband.hip: the two grids, the
// choice between the chain's forms, the dispatch on the channel count, the colour pre-pass of a scheduled shutter and the
// step rule of the viewports.  Host code only.
#ifndef VM_CHAIN_LAUNCH_H
#define VM_CHAIN_LAUNCH_H

#include <type_traits>
#include "vm_chain.h"
#include "vm_warp.h"     // vm_render_window_form, VmTransition, vm_launch_rates, VM_WARP_CANVAS

namespace vm_chain {

struct Grid { dim3 g, b; };

// the plain grid of a w x h output: 64 x 4 pixels per workgroup, one per thread
inline Grid plain_grid(int w, int h) { return {dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4)}; }

// the window grid of a w x h OUTPUT (vm_chain_win.h): tiles of RW x RH pixels, counted into A.tiles_x / A.ntiles, and a
// whole number of workgroups per XCD
template <class Args> Grid window_grid(Args &A, int w, int h)
{
    A.tiles_x = (w + RW - 1) / RW;
    A.ntiles = A.tiles_x * ((h + RH - 1) / RH);
    return {dim3(((A.ntiles + 7) / 8) * 8), dim3(RW, RH)};
}

// one launch over a w x h output with the kernels of one channel count: the plain form, or the window form with or
// without a path (A.uf)
template <class Args>
void launch_form(bool window, int w, int h, Args &A, void (*plain)(Args), void (*win_u)(Args), void (*win)(Args), hipStream_t s)
{
    const Grid G = window ? window_grid(A, w, h) : plain_grid(w, h);
    void (*const k)(Args) = !window ? plain : A.uf ? win_u : win;
    hipLaunchKernelGGL(k, G.g, G.b, 0, s, A);
}

// f(Channels<C>{}) for the call's tail: MAPS, 0 is the maps tail; 1..4 are layers; anything else is the canvas tail, if
// the caller has one
template <int C> using Channels = std::integral_constant<int, C>;
template <bool MAPS = false, bool CANVAS_TAIL = true, class F> void for_channels(int channels, F &&f)
{
    if constexpr (MAPS)
        if (channels == 0)
            return f(Channels<0>{});
    switch (channels) {
    case 1: f(Channels<1>{}); break;
    case 2: f(Channels<2>{}); break;
    case 3: f(Channels<3>{}); break;
    case 4: f(Channels<4>{}); break;
    default:
        if constexpr (CANVAS_TAIL) f(Channels<VM_WARP_CANVAS>{});
        break;
    }
}

// the pre-pass of a shutter under a schedule: K into the .y of the rate plane (its .x, the geometry at t_color, is not read)
template <class Args> void launch_colour_rates(const Args &A, hipStream_t s)
{
    VmTransition T{};
    T.w = A.w; T.h = A.h; T.rs = A.rs;
    T.t = A.t_color; T.ease = A.ease;
    T.sched_geo = A.sched_geo; T.sched_color = A.sched_color; T.rates = A.rates;
    vm_launch_rates(T, s);
}

// vm_render_window_form for a viewport: the window form takes steps up to 1 (step <= 1 rather than !(step > 1): anything
// the host let through that is no step up to 1 is plain)
template <class Args> bool viewport_window_form(const Args &A)
{
    return vm_render_window_form(A.rs, A.h) && A.step_x <= 1.0f && A.step_y <= 1.0f;
}

} // namespace vm_chain

#endif
