// vm_filter.h -- the launcher of vm_filter.hip, called from vm_render_calls.cpp.
#ifndef VM_FILTER_H
#define VM_FILTER_H

#include "vm_viewport.h"

// One filtered viewport call (vm_filter.hip): a viewport call whose last taps -- the ones that read a canvas
// or a layer -- go through a cubic filter of 4 x 4 texels.  The seven coefficients are the filter's two polynomials
//   inner(d) = ((p3 * d + p2) * d) * d + p0                 for the two texels next to the sample, 0 <= d <= 1
//   outer(d) = ((q3 * d + q2) * d + q1) * d + q0            for the two beyond them,                1 <= d <= 2
// (the host's table, vm_render_calls.cpp): one kernel serves every cubic filter.  Everything else is VmViewport's.
struct VmFiltered : VmViewport {
    float p3, p2, p0, q3, q2, q1, q0;
};
void vm_launch_filtered(const VmFiltered &V, hipStream_t s);

#endif
