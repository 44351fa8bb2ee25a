// vm_track.h -- the point tracker of stage 2 (MdiEditor::AddPoint / MovePoint / Histo,
// UI/MdiEditor.cpp:1230-1393, 1516-1582): the full-resolution frames and flows of a video pair
// (MdiEditor's resample1/2, f1/f2, b1/b2) and the launcher of vm_track.hip.  DESIGN.md 3.7.
#ifndef VM_TRACK_H
#define VM_TRACK_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vmorph.h"

// every segment i (checked by the host: a blend has ofr != frame, a chain dir = +-1) writes
// out[i * depth + s] for each frame s it covers (one wave64 per segment); frame0/1: depth RGBA8
// frames of w x h, f0/f1, b0/b1: depth flows (float2, tight) of video 0 / 1
void vm_track_launch(const vm_track_segment *seg, int n, const uchar4 *frame0, const uchar4 *frame1, const float2 *f0,
                     const float2 *f1, const float2 *b0, const float2 *b1, int w, int h, int depth, vm_track_point *out,
                     hipStream_t s);
// RGB8 rows (pitch bytes) -> tight RGBA8
void vm_track_launch_rgba(const uint8_t *rgb, int pitch, int w, int h, uchar4 *out, hipStream_t s);

// Bounds that keep every position a step can reach an int, so the kernel's and the spec's conversions agree:
// |key| <= 1e6, |flow| <= 1e5, depth <= 16384 give |x| <= 1e6 + 16383 (1e5 + 1) < 1.7e9.  Uploaded flows
// beyond them (or not finite) and keys beyond them are VM_E_INVALID; computed flows are not checked.
#define VM_TRACK_MAX_KEY 1000000
#define VM_TRACK_MAX_FLOW 1.0e5f
#define VM_TRACK_MAX_DEPTH 16384

// ---- host side (vm_track.cpp) ------------------------------------------------------------------
#include "vm_devmem.h"
#include <vector>

struct vm_ctx;

struct vm_track {
    vm_ctx *ctx = nullptr;
    int device = 0;                       // of ctx: the buffers can be freed after the context is gone
    int w = 0, h = 0, depth = 0;
    VmDev<uchar4> frames[2];              // resample1 / resample2: depth frames each, RGBA8
    VmDev<float2> f[2], b[2];             // f1 / f2, b1 / b2: depth flows each
    std::vector<char> has_frame[2], has_f[2], has_b[2]; // per frame: supplied yet?
};
#endif
