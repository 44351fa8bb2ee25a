// vm_shutter.hip -- motion blur for gfx950: the compositor's chain (kernel_render_halfway_image, Algorithm/render.cu:16-60;
// vm_chain.h, vm_chain_win.h) walked at the N sample times of a shutter per output pixel, the samples' colours summed in
// registers and stored once.  One launch per call, whatever N is.
//
// In float32, without contraction, for s = 0 .. N - 1 (1 <= N <= 64):
//   f   = ((float)s + 0.5f) / (float)N                                     correctly rounded division
//   t_s = fminf(fmaxf(geo_open + (geo_close - geo_open) * f, 0), 1)        a shutter across t = 0 or 1 holds still outside
//   (map0, map1)_s = the chain at geo_fa = t_s
//   c_s = the tail of the uniform call on them: the canvas taps of vm_render.hip (+ ex, then + 0.5f, tap_rgb's weights) or
//         the layer taps of vm_warp.hip, blended by color_from with the call's one color_fa (a dissolve is not motion)
//   acc = acc + c_s                                                        acc starts at +0, in sample order
// and the pixel is (uint8)((double)(acc / (float)N) + 0.5) per channel for the canvases, acc / (float)N for layers.  With
// N = 1 and geo_open == geo_close == g in [0, 1] that is the uniform call's result at g, bit for bit.
//
// The window form restages its LDS window sample by sample, because the window's origin follows t_s: a barrier before the
// restaging (every tap of the sample before has been served) as well as the one after it, and a thread without a pixel
// stays in the loop for both.  Two consecutive samples whose windows have the same origin share the staged texels -- the
// window holds exact texels, the bits cannot change -- which is the usual case for a short shutter (VM_SHUTTER_SKIP=0
// restages always: the A/B of profiles/shutter.md).
#include "vm_chain.h"
#include "vm_chain_launch.h"
#include "vm_shutter_tail.h"

#ifndef VM_SHUTTER_SKIP
#define VM_SHUTTER_SKIP 1
#endif

namespace {

using namespace vm_chain;

// the plain form: one pixel per thread, every tap a global gather
template <int C> __global__ __launch_bounds__(256) void k_shutter(const VmShutter A)
{
    const float n = (float)A.samples;
    float acc[NACC<C>] = {};
    int x = 0, y = 0;
    for (int s = 0; s < A.samples; ++s) {
        Landing L;
        if (!chain_plain<false>(A.w, A.h, A.rs, sample_time<true>(A.geo_open, A.geo_close, s, n), A.vf, A.uf, nullptr, x, y, L))
            return;
        add_sample<C>(A, L, per_sample(A.color_fa), acc);
    }
    store_mean<C>(A, x, y, acc, n);
}

// whether sample s stages the window at (ox, oy), for the whole workgroup: not if the sample before left it there; the
// barrier before a restaging is taken here (every tap of the sample before has been served)
// (not restage<false> of vm_shutter_tail.h: its `moved`, formed before the early return, moves all ten window kernels)
__device__ __forceinline__ bool restage(int s, int ox, int oy, int &at_x, int &at_y)
{
    ox = __builtin_amdgcn_readfirstlane(ox); oy = __builtin_amdgcn_readfirstlane(oy);
    if (VM_SHUTTER_SKIP && s && ox == at_x && oy == at_y)
        return false;
    if (s)
        __syncthreads();
    at_x = ox; at_y = oy;
    return true;
}

// the window form.  The chain's statements stand in the sample loop: a thread without a pixel goes on to the next
// sample's barriers, only the workgroup past the last tile leaves.  (x, y) belong to the chain's statements, so the one
// store stands behind the last sample inside the loop.
#define VM_CHAIN_WIN_NO_PIXEL continue
#define VM_CHAIN_WIN_STAGE(ox, oy) restage(s, ox, oy, at_x, at_y)
template <bool HAS_U, int C> __global__ __launch_bounds__(RW * RH) void k_shutter_win(const VmShutter A)
{
    constexpr bool RATES = false;       // (a shutter under a transition schedule is vm_tshutter.hip: RATES, ramped per sample)
    const float2 *rates = nullptr;
    const int rs = A.rs, ntiles = A.ntiles;
    const float2 *__restrict__ vf = A.vf, *__restrict__ uf = A.uf;
    float acc[NACC<C>] = {};
    int at_x = 0, at_y = 0;             // where the staged window is (read from the second sample on: restage())
    for (int s = 0; s < A.samples; ++s) {
        const int w = per_sample(A.w), h = per_sample(A.h), tiles_x = per_sample(A.tiles_x);
        const float n = (float)per_sample(A.samples);
        // (geo_open alone: close - open is then formed per sample, and close is read from its scalar register)
        const float geo_fa = sample_time<true>(per_sample(A.geo_open), A.geo_close, s, n);
#include "vm_chain_win.h"
        add_sample<C>(A, L, per_sample(A.color_fa), acc);
        if (s == A.samples - 1)
            store_mean<C>(A, x, y, acc, n);
    }
}
#undef VM_CHAIN_WIN_NO_PIXEL
#undef VM_CHAIN_WIN_STAGE

} // namespace

void vm_launch_shutter(const VmShutter &S, hipStream_t s)
{
    VmShutter A = S;
    for_channels(A.channels, [&](auto c) {
        constexpr int C = decltype(c)::value;
        launch_form(vm_render_window_form(A.rs, A.h), A.w, A.h, A, k_shutter<C>, k_shutter_win<true, C>, k_shutter_win<false, C>, s);
    });
}
