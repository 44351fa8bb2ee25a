// vm_error.h -- the error view of a level: the per-pixel energy terms the solver minimises, their five
// totals, and the heat-ramp image of one of them.  Shared between vm_error.hip (kernels) and vm_error.cpp (C-ABI).
#ifndef VM_ERROR_H
#define VM_ERROR_H

#include "vm_internal.h"

// One level (or one page of a video level) as k_error_terms reads it: the arrays vm_level_get_field returns for
// VM_F_VALUE, VM_F_V, VM_F_TPS_B, VM_F_UI_AXY, VM_F_UI_B and -- temp_mask != nullptr <=> the page is swept with
// flag == true -- VM_F_TEMP_REF / VM_F_TEMP_MASK; plane[k] (VM_ERR_*): where term k of every pixel goes (rows of the
// level's stride), or nullptr.
struct VmErrJob {
    const float *value, *ui_axy, *temp_mask;
    const float2 *v, *tps_b, *ui_b, *temp_ref;
    float factor_d;
    float *plane[5];
};

// A workgroup folds 64 x 4 pixels; 32 workgroups share an arrival counter, each counter on a 128-byte line of its own
#define VM_ERR_BW 64
#define VM_ERR_BH 4
#define VM_ERR_TK_GROUP 32
#define VM_ERR_TK_STRIDE 32
inline int vm_error_blocks(int w, int h) { return ((w + VM_ERR_BW - 1) / VM_ERR_BW) * ((h + VM_ERR_BH - 1) / VM_ERR_BH); }
// arrival counters of one pair, in words: the top counter and one per group
inline size_t vm_error_ticket_words(int nblk) { return (size_t)((nblk + VM_ERR_TK_GROUP - 1) / VM_ERR_TK_GROUP + 1) * VM_ERR_TK_STRIDE; }

// ONE launch for n levels of one geometry (blockIdx.z = pair): planes as the jobs ask, part = n x blocks x 5 partial
// sums, tickets = n x vm_error_ticket_words(blocks) words the caller zeroed, totals = n x 5 (pair-major)
void vm_launch_error_terms(const VmErrJob *jobs_dev, int n, int w, int h, int rs, float inv_wh, const vm_kern_params &kp,
                           double *part, unsigned *tickets, double *totals, hipStream_t s);
// term `what` of the level sampled to w0 x h0 as k_upscale samples v, times gain, through the heat ramp: RGB8 rows of
// pitch_bytes
void vm_launch_error_image(const VmErrJob &job, int w, int h, int rs, float inv_wh, const vm_kern_params &kp, int what,
                           float gain, int w0, int h0, uint8_t *rgb, int pitch_bytes, hipStream_t s);

#endif
