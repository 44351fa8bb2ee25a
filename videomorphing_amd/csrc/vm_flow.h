// vm_flow.h -- launchers of vm_flow.hip: dense optical flow (Farneback's polynomial expansion,
// DESIGN.md 3.6), the flow MdiEditor::OpticalFlow computes (UI/MdiEditor.cpp:1584-1689).
#ifndef VM_FLOW_H
#define VM_FLOW_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// constants of the polynomial expansion for one (poly_n, poly_sigma): 1-D weights g(t), t = -n..n,
// and the pieces of the inverse Gram matrix (b = S_x * ib, A_xy = S_xy * ixy,
// A_xx = q0 S_1 + q1 S_xx + q2 S_yy, A_yy = q0 S_1 + q2 S_xx + q1 S_yy)
struct VmPolyConst {
    int n;
    float g[7];
    float ib, ixy, q0, q1, q2;
};

// grey planes (w x h floats, tight)
void vm_flow_launch_grey_rgb(const uint8_t *rgb, int pitch_bytes, int w, int h, float *out, hipStream_t s);
void vm_flow_launch_grey_rgba(const uchar4 *rgba, int w, int h, float *out, hipStream_t s);
// separable blur (reflect-101) of a w x h plane with 2r+1 taps (device array); tmp: w x h scratch
void vm_flow_launch_blur(const float *src, float *tmp, float *dst, int w, int h, const float *taps, int r, hipStream_t s);
// bilinear resize W x H -> w x h (source coordinate (x + 0.5) W / w - 0.5, clamped)
void vm_flow_launch_resize(const float *src, int W, int H, float *dst, int w, int h, hipStream_t s);
// polynomial expansion of a w x h plane -> p0 = (b_x, b_y, A_xx, A_yy), p1 = A_xy
void vm_flow_launch_poly(const float *img, int w, int h, const VmPolyConst &pc, float4 *p0, float *p1, hipStream_t s);
// one iteration at one scale for nflows flows (blockIdx.z): pairs[f] = (slot of frame a, slot of frame b);
// frame slot i's planes at p0 + i * plane, p1 + i * plane; flow f's d at d_in / d_out + f * plane
void vm_flow_launch_iter(const float4 *p0, const float *p1, size_t plane, const int2 *pairs, int nflows,
                         const float2 *d_in, float2 *d_out, int w, int h, int win, hipStream_t s);
// d at the finer scale: bilinear resize of every flow's field (W x H -> w x h) times `mul`
void vm_flow_launch_resize_flow(const float2 *src, int W, int H, float2 *dst, int w, int h, float mul, int nflows,
                                hipStream_t s);

// ---- host side (vm_flow.cpp) -------------------------------------------------------------------
#include <functional>
#include <vector>
#include "../../include/vmorph.h"

struct vm_ctx;

// Per-call working set, bounded by VM_FLOW_BUDGET: per frame 20 B per pixel of every scale (the
// polynomial planes, ~26.7 B per full-resolution pixel at pyr_scale 0.5), per flow 16 B per
// full-resolution pixel (d, ping-pong) plus the caller's 8 B output; four full-resolution float
// planes of scratch.  A call with more frames works through them in chunks.
#define VM_FLOW_BUDGET (4ull << 30)
#define VM_FLOW_MAX_BLUR_R 96 // LDS column tile of the scale blur: (64 + 2 r) x 64 floats <= 64 KiB

// p == NULL: the defaults; checks the parameters and the frame size (VM_E_INVALID with a message)
int vm_flow_resolve(const vm_flow_params *p, int w, int h, vm_flow_params *out, const char *fn);
size_t vm_flow_frame_bytes(int w, int h, const vm_flow_params &p);
size_t vm_flow_flow_bytes(int w, int h);

// one chunk: every frame expanded once, every pair solved in the same launches.  src(i, dst) writes
// frame i's grey plane (w x h floats, tight) on the context's stream; a pair's `out` is a device
// array of w x h float2 (tight).  Returns with the stream drained.
struct VmFlowPair {
    int a, b;
    float2 *out;
};
using VmFlowSource = std::function<int(int frame, float *dst)>;
int vm_flow_run(vm_ctx *c, int w, int h, const vm_flow_params &p, int nframes, const VmFlowSource &src,
                const std::vector<VmFlowPair> &pairs);
// The flows along two videos of d frames each (MdiEditor::OpticalFlow, UI/MdiEditor.cpp:1584-1689), walked in chunks
// [t0, t1] that share their end frame and fit VM_FLOW_BUDGET with both families: the forward flow of (video k, frame
// t) is computed in the chunk with t0 <= t < t1 and lands in fwd(k, t), the backward flow in the chunk with
// t0 < t <= t1 and lands in bwd(k, t) (bwd empty: forward flows only), each exactly once; fwd(k, d - 1) and bwd(k, 0)
// are never asked for.  src(k, t, dst) writes the frame's grey plane as for vm_flow_run.
using VmFlowVideoSource = std::function<int(int video, int frame, float *dst)>;
using VmFlowVideoOut = std::function<float2 *(int video, int frame)>;
int vm_flow_run_videos(vm_ctx *c, int w, int h, int d, const vm_flow_params &p, const VmFlowVideoSource &src,
                       const VmFlowVideoOut &fwd, const VmFlowVideoOut &bwd);
#endif
