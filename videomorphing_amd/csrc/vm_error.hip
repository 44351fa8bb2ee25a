// vm_error.hip -- the error view the reference's UI promises and never computes ("Error Image",
// UI/MdiEditor.cpp:348-373, 1928-1933): per pixel the terms of the energy the sweep minimises (the per-pixel terms of
// Algorithm/morph.cu:730-761), their totals, and a heat-ramp image of one of them.  DESIGN.md 3.8 states the
// arithmetic; tests/error_ref.py restates it in numpy.
//
//   k_error_terms  one launch per call, blockIdx.z = pair: reads the level's arrays once (32 B per pixel, 44 B with
//                  the temporal term), writes the planes that were asked for and folds the five sums in the same pass
//   k_error_image  RGB8 of w0 x h0: the chosen term at the taps of k_upscale (vm_render.hip), recomputed from the
//                  level's arrays on the fly, blended, times gain, through the ramp
//
// Arithmetic: float32 planes, IEEE basic operations in the stated order, no contraction, the same in every math mode.
// Totals: doubles, folded in ONE order that the level's geometry fixes (the discipline of DESIGN.md 3.4) -- a
// butterfly inside each wave, the four waves in sequence, one partial per workgroup; the workgroup that arrives last
// folds the partials in index order.  Partials cross workgroups the way vm_sync.hip's brick partials do: write-through
// stores, a drain, an integer arrival ticket; no atomic ever touches a floating-point value.
#include "vm_error.h"

#pragma clang fp contract(off)

namespace {

struct Terms {
    float e[5];
};

__device__ __forceinline__ Terms terms_at(const VmErrJob &J, int x, int y, int rs, float inv_wh, const vm_kern_params &P)
{
    const size_t i = (size_t)y * rs + x;
    const float value = J.value[i], axy = J.ui_axy[i];
    const float2 v = J.v[i], tb = J.tps_b[i], ub = J.ui_b[i];
    Terms t;
    t.e[VM_ERR_SSIM] = (P.w_ssim * (1.0f - value)) * inv_wh;
    t.e[VM_ERR_TPS] = P.w_tps * (0.5f * (v.x * tb.x + v.y * tb.y));
    t.e[VM_ERR_UI] = axy > 0 ? (P.w_ui * ((ub.x * ub.x + ub.y * ub.y) / (4.0f * axy))) * inv_wh : 0.0f;
    t.e[VM_ERR_TEMP] = 0.0f;
    if (J.temp_mask) {
        const float2 ref = J.temp_ref[i];
        t.e[VM_ERR_TEMP] = (((P.w_temp * (fabsf(v.x - ref.x) + fabsf(v.y - ref.y))) * J.temp_mask[i]) * J.factor_d) * inv_wh;
    }
    t.e[VM_ERR_ALL] = ((t.e[VM_ERR_SSIM] + t.e[VM_ERR_TPS]) + t.e[VM_ERR_UI]) + t.e[VM_ERR_TEMP];
    return t;
}

__device__ __forceinline__ double wave_butterfly(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// the five sums over the 256 threads: butterfly inside each wave, the four waves in sequence; thread k < 5 returns sum k
__device__ __forceinline__ double block_fold(const double (&acc)[5], double (*red)[5], int tid)
{
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double s = wave_butterfly(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    double t = 0;
    if (tid < 5) t = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(256) void k_error_terms(const VmErrJob *__restrict__ jobs, int w, int h, int rs, float inv_wh,
                                                     vm_kern_params P, double *part, unsigned *tickets, double *totals)
{
    __shared__ double red[4][5];
    __shared__ int s_last;
    const VmErrJob J = jobs[blockIdx.z];
    const int x = blockIdx.x * VM_ERR_BW + threadIdx.x, y = blockIdx.y * VM_ERR_BH + threadIdx.y;
    const int tid = threadIdx.y * VM_ERR_BW + threadIdx.x;
    double acc[5] = {0, 0, 0, 0, 0};
    if (x < w && y < h) {
        const Terms t = terms_at(J, x, y, rs, inv_wh, P);
        const size_t i = (size_t)y * rs + x;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (J.plane[k]) J.plane[k][i] = t.e[k];
            acc[k] = (double)t.e[k];
        }
    }
    const int nblk = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
    double *mine = part + (size_t)blockIdx.z * nblk * 5;
    const double sum = block_fold(acc, red, tid);
    // publish: write-through, drained by the storing wave (threads 0..4 and the ticket taker share wave 0)
    if (tid < 5)
        __hip_atomic_store((unsigned long long *)&mine[(size_t)lin * 5 + tid], (unsigned long long)__double_as_longlong(sum),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        const int ngr = (nblk + VM_ERR_TK_GROUP - 1) / VM_ERR_TK_GROUP, grp = lin / VM_ERR_TK_GROUP;
        const unsigned gsize = (unsigned)min(VM_ERR_TK_GROUP, nblk - grp * VM_ERR_TK_GROUP);
        unsigned *tk = tickets + (size_t)blockIdx.z * (ngr + 1) * VM_ERR_TK_STRIDE;
        unsigned *gt = tk + (size_t)(1 + grp) * VM_ERR_TK_STRIDE;
        int last = 0;
        // two levels, as in vm_sync.hip: arrivals on ONE line serialise, so 32 workgroups share a counter and the last
        // of a group arrives at the pair's top counter (the host zeroes the counters ahead of every launch)
        if (__hip_atomic_fetch_add(gt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1)
            last = ngr == 1 || __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)ngr - 1;
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    // the last workgroup of the pair: thread t takes partials t, t + 256, ... in sequence, then the block's fold
    double tot[5] = {0, 0, 0, 0, 0};
    for (int b = tid; b < nblk; b += 256)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const unsigned long long u = __hip_atomic_load((const unsigned long long *)&mine[(size_t)b * 5 + k], __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
            tot[k] += __longlong_as_double((long long)u);
        }
    const double total = block_fold(tot, red, tid);
    if (tid < 5) totals[(size_t)blockIdx.z * 5 + tid] = total;
}

// the sampling of k_upscale (vm_render.hip; BiLinear of MatchingThread.cpp:103-136) on a scalar plane that is NOT
// rescaled by the size ratio, then gain, clamp and the heat ramp
__global__ __launch_bounds__(256) void k_error_image(VmErrJob J, int w, int h, int rs, float inv_wh, vm_kern_params P, int what,
                                                     float gain, int w0, int h0, uint8_t *__restrict__ rgb, int pitch)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w0 || y >= h0)
        return;
    float s;
    if (w == w0 && h == h0) {
        s = terms_at(J, x, y, rs, inv_wh, P).e[what]; // ratio 1: copied
    } else {
        const float fy = (float)((y + 0.5) / h0 * h - 0.5);
        const float fx = (float)((x + 0.5) / w0 * w - 0.5);
        const int xi[2] = {(int)floorf(fx), (int)ceilf(fx)};
        const int yi[2] = {(int)floorf(fy), (int)ceilf(fy)};
        const float uu = fx - xi[0], vv = fy - yi[0];
        float val[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int tx = min(max(xi[i], 0), w - 1), ty = min(max(yi[j], 0), h - 1);
                val[i][j] = terms_at(J, tx, ty, rs, inv_wh, P).e[what];
            }
        s = val[0][0] * (1 - uu) * (1 - vv) + val[0][1] * (1 - uu) * vv + val[1][0] * uu * (1 - vv) + val[1][1] * uu * vv;
    }
    const float t = fminf(fmaxf(s * gain, 0.0f), 1.0f);
    const float r = fminf(3.0f * t, 1.0f);
    const float g = fminf(fmaxf(3.0f * t - 1.0f, 0.0f), 1.0f);
    const float b = fminf(fmaxf(3.0f * t - 2.0f, 0.0f), 1.0f);
    uint8_t *o = rgb + (size_t)y * pitch + 3 * x;
    o[0] = (uint8_t)(r * 255.0f + 0.5f);
    o[1] = (uint8_t)(g * 255.0f + 0.5f);
    o[2] = (uint8_t)(b * 255.0f + 0.5f);
}

} // namespace

void vm_launch_error_terms(const VmErrJob *jobs_dev, int n, int w, int h, int rs, float inv_wh, const vm_kern_params &kp,
                           double *part, unsigned *tickets, double *totals, hipStream_t s)
{
    dim3 b(VM_ERR_BW, VM_ERR_BH), g((w + VM_ERR_BW - 1) / VM_ERR_BW, (h + VM_ERR_BH - 1) / VM_ERR_BH, n);
    hipLaunchKernelGGL(k_error_terms, g, b, 0, s, jobs_dev, w, h, rs, inv_wh, kp, part, tickets, totals);
}

void vm_launch_error_image(const VmErrJob &job, int w, int h, int rs, float inv_wh, const vm_kern_params &kp, int what,
                           float gain, int w0, int h0, uint8_t *rgb, int pitch_bytes, hipStream_t s)
{
    dim3 b(64, 4), g((w0 + 63) / 64, (h0 + 3) / 4);
    hipLaunchKernelGGL(k_error_image, g, b, 0, s, job, w, h, rs, inv_wh, kp, what, gain, w0, h0, rgb, pitch_bytes);
}
