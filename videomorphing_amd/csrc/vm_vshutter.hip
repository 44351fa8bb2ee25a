// vm_vshutter.hip -- viewports over a shutter, uniformly and under a transition schedule, for gfx950: the
// compositor's chain (kernel_render_halfway_image, Algorithm/render.cu:16-60; vm_chain.h, vm_chain_win.h) started from the
// nx x ny sub-sample points of every pixel of an output grid laid freely over the halfway domain, at the T
// sample times of a shutter, with per-texel rates ramped at each of them under a schedule.  One
// launch per call (and the one pre-pass under a schedule), whatever T and N = nx * ny are, and no device memory that grows
// with either.
//
// In float32, without contraction, for output pixel (X, Y); time sample tau = 0 .. T - 1 is the OUTER loop, sub-sample
// s = j * nx + i = 0 .. N - 1 the INNER one, i fastest (1 <= T <= 64, 1 <= N <= 64, T * N <= 256):
//   f_tau = ((float)tau + 0.5f) / (float)T                                  correctly rounded division
//   q     = (qx, qy) of vm_viewport.hip for (X, Y, i, j), unchanged
//   uniform:    t_tau = fminf(fmaxf(geo_open + (geo_close - geo_open) * f_tau, 0), 1)
//               (p, V) = the chain from q at geo_fa = t_tau;  c = the uniform tail, blended by color_from with color_fa
//   scheduled:  K = ramp(schedule_colour, t_color, ease)                    once per call: a dissolve is not motion
//               t_tau = t_open + (t_close - t_open) * f_tau                 not clamped: ramp clamps per texel
//               (p, V) = the chain from q under G_tau = ramp(schedule_geometry, t_tau, ease), g = tapr(G_tau, p) anew at
//               every p;  k = tapr(K, p);  c = the transition tail, blended by color_from with k
//   acc = acc + c                                                           acc starts at +0, in loop order
// and the pixel is (uint8)((double)(acc / (float)(T * N)) + 0.5) per channel for the canvases, acc / (float)(T * N) for
// layers.  With T = 1 that is vm_viewport.hip's result, with {0, 0, 1, 1, w, h, 1, 1} vm_shutter.hip's or vm_tshutter.hip's,
// bit for bit.
//
// The window form runs for steps up to 1, as in vm_viewport.hip (viewport_window_form, vm_chain_launch.h).  Its window belongs to the tile AND to the time sample:
// sub-sample 0 of a time sample alone may stage, by the shutters' rules -- a barrier before a restaging from the second
// time sample on (every tap of every sub-sample of the time before has been served); uniform: no restaging where the
// origin has not moved; scheduled: (G, K) at every time sample, v and u only where the origin has moved -- and the
// sub-samples after it tap what is there, with no barrier.  A thread without a pixel stays in both loops for the
// barriers of the time samples to come; only the workgroup past the last tile leaves.
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_ramp.h"
#include "vm_shutter_tail.h"        // sample_time, restage
#include "vm_viewport_win.h"        // sample_q, cell_at, Out, next_sub, and the hooks of the window form
#include "vm_vshutter.h"

namespace {

using namespace vm_chain;

// what the chain takes in the place of its rate plane at time t: the geometry schedule ramped where it is read, or nothing
template <bool RATES> __device__ __forceinline__ auto rates_at_time(const VmVShutter &A, float t)
{
    if constexpr (RATES)
        return Ramped{A.sched_geo, A.rates, t, A.ease};
    else
        return (const float2 *)nullptr;
}

// the plain form: one output pixel per thread, every tap a global gather, every rate texel ramped where it is read; any step
template <int C, bool RATES> __global__ __launch_bounds__(256) void k_vblur(const VmVShutter A)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.out_w || y >= A.out_h)
        return;
    const float nt = (float)A.samples, nx = (float)A.nx, ny = (float)A.ny;
    float acc[NACC<C>] = {};
    for (int ts = 0; ts < A.samples; ++ts) {
        const float t = sample_time<!RATES>(A.t_open, A.t_close, ts, nt);     // clamped where it is the chain's geo_fa
        const auto rates = rates_at_time<RATES>(A, t);
        for (int j = 0; j < A.ny; ++j)
            for (int i = 0; i < A.nx; ++i) {
                Landing L;
                chain_plain_from<RATES>(A.w, A.h, A.rs, RATES ? 0.0f : t, A.vf, A.uf, rates, sample_q(A.x0, A.step_x, x, i, nx),
                                        sample_q(A.y0, A.step_y, y, j, ny), L);
                add_sample<C>(A, L, RATES ? L.k : per_sample(A.color_fa), acc);
            }
    }
    store_mean<C>(Out{A.out_w, A.rgb, A.out}, x, y, acc, (float)(A.samples * A.nx * A.ny));
}

// the window form.  The chain's statements stand in the inner loop with the shutters' hooks and the viewport's
// (vm_viewport_win.h); sub-sample 0 of a time sample alone may stage, by restage<RATES> of vm_shutter_tail.h: a thread
// without a pixel goes on through both loops (the counters are kept in the loop's own increment, which `continue` reaches)
// to the barriers of the time samples to come, only the workgroup past the last tile leaves, and the one store stands
// behind the last sample inside the loop.  x, y, tiles_x and ntiles count output pixels and tiles.
#define VM_CHAIN_WIN_NO_PIXEL continue
#define VM_CHAIN_WIN_STAGE(ox, oy) (s == 0 && restage<RATES>(ts, ox, oy, at_x, at_y, moved))
#define VM_CHAIN_WIN_STAGE_FIELD moved
template <bool HAS_U, int C, bool RATES> __global__ __launch_bounds__(RW * RH) void k_vblur_win(const VmVShutter A)
{
    const int rs = A.rs, ntiles = A.ntiles;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf;
    const int subs = A.nx * A.ny;
    float acc[NACC<C>] = {};
    int at_x = 0, at_y = 0;             // where the staged window is (read from the second time sample on: restage())
    bool moved = true;
    for (int ts = 0; ts < A.samples; ++ts) {
        int si = 0, sj = 0;
        for (int s = 0; s < subs; ++s, next_sub(si, sj, A.nx)) {
            const int w = per_sample(A.w), h = per_sample(A.h), tiles_x = per_sample(A.tiles_x);
            const float t = sample_time<!RATES>(per_sample(A.t_open), A.t_close, ts, (float)per_sample(A.samples));
            const float geo_fa = RATES ? 0.0f : t;      // (under RATES every round takes its own g)
            const auto rates = rates_at_time<RATES>(A, t);
#include "vm_chain_win.h"
            add_sample<C>(A, L, RATES ? L.k : per_sample(A.color_fa), acc);
            if (ts == A.samples - 1 && s == subs - 1)
                store_mean<C>(Out{A.out_w, A.rgb, A.out}, x, y, acc, (float)per_sample(A.samples * subs));
        }
    }
}
#undef VM_CHAIN_WIN_NO_PIXEL
#undef VM_CHAIN_WIN_STAGE
#undef VM_CHAIN_WIN_STAGE_FIELD
#include "vm_viewport_win.h"        // (the hooks leave)

template <bool RATES> void launch_channels(VmVShutter &A, hipStream_t s)
{
    for_channels(A.channels, [&](auto c) {
        constexpr int C = decltype(c)::value;
        launch_form(viewport_window_form(A), A.out_w, A.out_h, A, k_vblur<C, RATES>, k_vblur_win<true, C, RATES>, k_vblur_win<false, C, RATES>, s);
    });
}

} // namespace

void vm_launch_vshutter(const VmVShutter &S, hipStream_t s)
{
    VmVShutter A = S;
    if (!A.sched_geo) {
        launch_channels<false>(A, s);
        return;
    }
    launch_colour_rates(A, s);
    launch_channels<true>(A, s);
}
