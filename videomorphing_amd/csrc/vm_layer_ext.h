// vm_layer_ext.h -- launchers of vm_layer_ext.hip (Poisson boundary extension of float layers), called from
// vm_poisson_api.cpp.
#ifndef VM_LAYER_EXT_H
#define VM_LAYER_EXT_H

#include "vm_internal.h"

struct VmV3;

// the (ch, cw, C) canvas of a tight (h, w, C) layer: the layer at (ex, ex), zeros around it; valid = 1 on the image
void vm_layer_ext_launch_canvas(float *ext, uint8_t *valid, const float *tight, int C, int w, int h, int ex, hipStream_t s);
// the geometric type map: 2 outside the image, 1 on the image's outermost ring (where the canvas has cells beyond it), else 0
void vm_layer_ext_launch_type(uint8_t *type, int w, int h, int ex, hipStream_t s);
// every type-2 cell from the other side's tight layer, where the chain of the halfway field lands (valid = 1), or a hole
void vm_layer_ext_launch_fill(float *ext, uint8_t *valid, const uint8_t *type, const float *other, const float2 *v, int C, int w,
                              int h, int rs, int ex, int sign, hipStream_t s);
// right-hand side + initial guess of channels c0 .. c0 + n - 1 (n <= 3; the other lanes zero) on the solver's 12-byte
// vectors; *nz is raised by a right-hand side entry that is not zero
void vm_layer_ext_launch_setup(const float *ext, const uint8_t *valid, const uint8_t *type, VmV3 *B, VmV3 *X, int *nz, int cw,
                               int ch, int C, int c0, int n, hipStream_t s);
// the solution of those channels into every type > 0 cell, as it is; set_valid: and all of their valid become 1
void vm_layer_ext_launch_paste(float *ext, uint8_t *valid, const uint8_t *type, const VmV3 *X, int cw, int ch, int C, int c0,
                               int n, int set_valid, hipStream_t s);

#endif
