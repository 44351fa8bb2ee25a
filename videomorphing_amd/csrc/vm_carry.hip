// vm_carry.hip -- points and motion vectors carried through the morph, for gfx950: where a point of the
// output frame at one time lies at other times.  The chain of kernel_render_halfway_image (Algorithm/render.cu:16-60;
// UI/RenderWidget.cpp:229-266) started from a point q of the output frame at the from-time finds the halfway point p with
// q = p + s1 V + s2 U; from p the position at any time g is closed form, in float32 and in this order:
//   s1 = 2 g - 1;  s2 = 4 g - 4 g g;  out = ((px + s1 V.x) + s2 U.x, (py + s1 V.y) + s2 U.y)
// (the s2 term is added without a path too, U = 0, as the chain subtracts it).  Image 0 is time 0 and image 1 is time 1:
//   halfway = (px, py);  pos0 = (px - V.x, py - V.y);  pos1 = (px + V.x, py + V.y)
//   resid = fmaxf(|px20 - px19|, |py20 - py19|);  flags bit 0 / 1: pos0 / pos1 within [0, w - 1] x [0, h - 1]
// Under a schedule (RATES) the chain runs on the rate plane k_rates has ramped at the from-time, and the
// rate of a to-time t_k is the chain's own rate tap at p with the ramp taken at t_k: the four geometry-schedule texels
// are read once (GeoTap, vm_ramp.h) and ramped per to-time; no to-time rate plane is stored.
//
// The chain is vm_chain.h's, unchanged.  The points kernels walk chain_plain_from, one thread per point, every tap a
// global gather: 21 dependent gathers per point and nothing to hide them behind, so a call is bound by that latency
// like k_track (vm_track.hip), whatever n is below a full device -- it is not tuned.  Stores are laid out (nt, n, 2): a
// wave's stores of one to-time are contiguous.  The dense kernels ("motion maps") start from the pixel centres of the
// output frame and walk either form of the chain, as every render family does: chain_plain, or the window form of
// vm_chain_win.h with its defaults; the tail is the same loop over the to-times, into (nt, h, w, 2).  The to-times
// travel in the kernel argument and are read with scalar loads.
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_ramp.h"
#include "vm_carry.h"

namespace {

using namespace vm_chain;

// the tail of every kernel for the landing L of start point `at` of n: everything but the to-times first, then the loop
template <bool RATES> __device__ __forceinline__ void carry_tail(const VmCarry &A, size_t at, size_t n, const Landing &L)
{
    const float m0x = L.px - L.v.x, m0y = L.py - L.v.y;
    const float m1x = L.px + L.v.x, m1y = L.py + L.v.y;
    if (A.halfway) A.halfway[at] = make_float2(L.px, L.py);
    if (A.pos0) A.pos0[at] = make_float2(m0x, m0y);
    if (A.pos1) A.pos1[at] = make_float2(m1x, m1y);
    if (A.resid) A.resid[at] = fmaxf(fabsf(L.px - L.lx), fabsf(L.py - L.ly));
    if (A.flags) {
        const float xm = (float)(A.w - 1), ym = (float)(A.h - 1);
        const bool in0 = 0.0f <= m0x && m0x <= xm && 0.0f <= m0y && m0y <= ym;
        const bool in1 = 0.0f <= m1x && m1x <= xm && 0.0f <= m1y && m1y <= ym;
        A.flags[at] = (uint8_t)((in0 ? 1 : 0) | (in1 ? 2 : 0));
    }
    if (!A.out)
        return;
    GeoTap gt{};
    if constexpr (RATES) gt = geo_tap_at(A.sched_geo, A.w, A.h, A.rs, L.px + 0.5f, L.py + 0.5f);
    float2 *o = A.out + at;
    for (int k = 0; k < A.nt; ++k, o += n) {
        float g = A.to[k];
        if constexpr (RATES) g = geo_rate(gt, g, A.ease);
        const float s1 = 2 * g - 1;
        const float s2 = 4 * g - 4 * g * g;
        *o = make_float2((L.px + s1 * L.v.x) + s2 * L.u.x, (L.py + s1 * L.v.y) + s2 * L.u.y);
    }
}

// the points: one thread per point (latency-bound by construction, see above)
template <bool HAS_U, bool RATES> __global__ __launch_bounds__(64) void k_carry_points(const VmCarry A)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= A.n)
        return;
    const float2 q = A.pts[i];
    Landing L;
    chain_plain_from<RATES>(A.w, A.h, A.rs, A.from, A.vf, HAS_U ? A.uf : nullptr, (const float2 *)A.rates, q.x, q.y, L);
    carry_tail<RATES>(A, (size_t)i, (size_t)A.n, L);
}

// the motion maps, plain form: one pixel per thread, every tap a global gather
template <bool RATES> __global__ __launch_bounds__(256) void k_motion(const VmCarry A)
{
    int x, y;
    Landing L;
    if (!chain_plain<RATES>(A.w, A.h, A.rs, A.from, A.vf, A.uf, (const float2 *)A.rates, x, y, L))
        return;
    carry_tail<RATES>(A, (size_t)y * A.w + x, (size_t)A.w * A.h, L);
}

// ... and the window form
template <bool HAS_U, bool RATES> __global__ __launch_bounds__(RW * RH) void k_motion_win(const VmCarry A)
{
    const int w = A.w, h = A.h, rs = A.rs, tiles_x = A.tiles_x, ntiles = A.ntiles;
    const float geo_fa = A.from;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf, *rates = A.rates;
#include "vm_chain_win.h"
    carry_tail<RATES>(A, (size_t)y * w + x, (size_t)w * h, L);
}

// the rate plane of a scheduled call, ramped at the from-time
void launch_from_rates(const VmCarry &C, hipStream_t s)
{
    VmTransition T{};
    T.w = C.w; T.h = C.h; T.rs = C.rs;
    T.t = C.from; T.ease = C.ease;
    T.sched_geo = C.sched_geo; T.sched_color = C.sched_color; T.rates = C.rates;
    vm_launch_rates(T, s);
}

} // namespace

void vm_launch_carry_points(const VmCarry &C, hipStream_t s)
{
    const bool rates = C.sched_geo != nullptr;
    if (rates) launch_from_rates(C, s);
    void (*const k)(VmCarry) = rates ? (C.uf ? k_carry_points<true, true> : k_carry_points<false, true>)
                                     : (C.uf ? k_carry_points<true, false> : k_carry_points<false, false>);
    hipLaunchKernelGGL(k, dim3(((unsigned)C.n + 63u) / 64u), dim3(64), 0, s, C);
}

void vm_launch_motion_maps(const VmCarry &C, hipStream_t s)
{
    VmCarry A = C;
    const bool window = vm_render_window_form(A.rs, A.h);
    if (A.sched_geo) {
        launch_from_rates(A, s);
        launch_form(window, A.w, A.h, A, k_motion<true>, k_motion_win<true, true>, k_motion_win<false, true>, s);
    } else {
        launch_form(window, A.w, A.h, A, k_motion<false>, k_motion_win<true, false>, k_motion_win<false, false>, s);
    }
}
