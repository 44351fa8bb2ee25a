// vm_carry.h -- the launchers of vm_carry.hip, called from vm_render_calls.cpp: points and motion vectors carried through
// the morph.
#ifndef VM_CARRY_H
#define VM_CARRY_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vmorph.h"

// (VM_CARRY_MAX_POINTS: 2^26 points per call -- 0.5 GB of start points, 0.5 GB per to-time; the grid and every byte count
// of a call stay far inside their types)
enum { VM_CARRY_MAX_TIMES = 64, VM_CARRY_MAX_DENSE_TIMES = 16, VM_CARRY_MAX_POINTS = 1 << 26 };

// One carry call.  The chain of vm_chain.h starts from the n points of pts (the points call) or from the w x h pixel
// centres of the output frame (the dense call: pts is not read, n is not read) at the from-time, and its landing is
// carried to the nt to-times.  Uniform (sched_geo == NULL): from / to are geo_fa values.  Under a schedule: from / to are
// times, the chain reads `rates` (the call's scratch plane, ramped at `from` by vm_launch_rates before the kernel) and
// the tail ramps the four geometry-schedule texels at the landing point per to-time.  Outputs, any may be NULL: out
// (nt, n, 2) or (nt, h, w, 2); halfway / pos0 / pos1 (n, 2), resid and flags n (the dense call: (h, w) each).
struct VmCarry {
    int w, h, rs;
    float from;
    int ease;
    const float2 *vf, *uf;
    const float2 *sched_geo, *sched_color;
    float2 *rates;
    const float2 *pts;
    int n;
    float2 *out, *halfway, *pos0, *pos1;
    float *resid;
    uint8_t *flags;
    int tiles_x, ntiles;            // the window form's (the launcher's)
    int nt;
    float to[VM_CARRY_MAX_TIMES];   // the to-times travel in the kernel argument
};

void vm_launch_carry_points(const VmCarry &C, hipStream_t s);
// the chain's form is chosen as vm_launch_warp chooses it (vm_render_window_form)
void vm_launch_motion_maps(const VmCarry &C, hipStream_t s);

#endif
