// vm_viewport_win.h -- what the kernels of an output grid laid freely over the halfway domain share,
// for vm_viewport.hip and vm_vshutter.hip: the point a sub-sample's chain starts from, the field cell under a tile's
// centre, the output grid as store_mean wants it, the sub-sample counter, and the hooks by which the window form
// (vm_chain_win.h) takes them.  Included before a unit's window kernel it defines the hooks, included again behind the
// kernel it takes them away.  The hooks read the kernel's A (x0, y0, step_x, step_y, nx, ny, out_w, out_h) and its
// sub-sample counters si, sj.
#ifndef VM_VIEWPORT_WIN_H
#define VM_VIEWPORT_WIN_H

#include "vm_chain.h"
#include "vm_shutter_tail.h"

namespace vm_chain {

// q of sub-sample i of n along one axis of output pixel X: the viewport's corner c0 and step
__device__ __forceinline__ float sample_q(float c0, float step, int X, int i, float n)
{
    return (c0 + ((float)X + sample_fraction(i, n)) * step) - 0.5f;
}

// the field cell nearest output edge `edge` (a tile's centre) along one axis; a corner far outside the field is cut off
// where the cell still is an int (the window then holds the field's clamped edge, or nothing useful)
__device__ __forceinline__ int cell_at(float c0, float step, int edge)
{
    return (int)rintf(__builtin_amdgcn_fmed3f((c0 + (float)edge * step) - 0.5f, -1e6f, 1e6f));
}

// where store_mean puts pixel (x, y): the tight output grid
struct Out { int w; uint8_t *rgb; float *out; };

// the next sub-sample s = sj * nx + si
__device__ __forceinline__ void next_sub(int &si, int &sj, int nx)
{
    if (++si == nx) {
        si = 0;
        ++sj;
    }
}

} // namespace vm_chain

#endif

#ifndef VM_CHAIN_WIN_Q_X
#define VM_CHAIN_WIN_Q_X sample_q(per_sample(A.x0), per_sample(A.step_x), x, si, (float)per_sample(A.nx))
#define VM_CHAIN_WIN_Q_Y sample_q(per_sample(A.y0), per_sample(A.step_y), y, sj, (float)per_sample(A.ny))
#define VM_CHAIN_WIN_ORIGIN_X (cell_at(A.x0, A.step_x, bx + RW / 2) - RW / 2)
#define VM_CHAIN_WIN_ORIGIN_Y (cell_at(A.y0, A.step_y, by + RH / 2) - RH / 2)
#define VM_CHAIN_WIN_CENTRE_X min(max(cell_at(A.x0, A.step_x, bx + RW / 2), 0), wm1)
#define VM_CHAIN_WIN_CENTRE_Y min(max(cell_at(A.y0, A.step_y, by + RH / 2), 0), hm1)
#define VM_CHAIN_WIN_OUTSIDE x >= per_sample(A.out_w) || y >= per_sample(A.out_h)
#else
#undef VM_CHAIN_WIN_Q_X
#undef VM_CHAIN_WIN_Q_Y
#undef VM_CHAIN_WIN_ORIGIN_X
#undef VM_CHAIN_WIN_ORIGIN_Y
#undef VM_CHAIN_WIN_CENTRE_X
#undef VM_CHAIN_WIN_CENTRE_Y
#undef VM_CHAIN_WIN_OUTSIDE
#endif
