// vm_track.hip -- key-point propagation for gfx950 (spec in tests/track_ref.py): the
// loops of MdiEditor::AddPoint / MovePoint (UI/MdiEditor.cpp:1230-1393) and the weight Histo
// (:1516-1582), for every segment of a call in ONE launch.
//
// One wave64 (one workgroup) per segment.  A segment is a chain of dependent flow gathers, so the
// launch is latency-bound: per step one uniform flow load, the step in double, then lanes 0-35 each
// load one pixel of the new point's 6 x 6 patch (RGBA8: one dword) and add it to an LDS count of the
// patch's 1000 bins.  The key histograms are built once into LDS.  With h1 the patch's counts and h2
// a key's: s1 = number of counted lanes, s11 = sum of h1 over the counted lanes' bins (= sum h1^2),
// s12 = sum of h2 over the same bins (= sum h1 h2).  Every sum is an integer reduction, exact and
// independent of the order; only the final correlation is double, with correctly rounded division
// and square root (this file is built with -ffp-contract=off).  A segment's bits do not depend on
// the other segments of its launch.
#include "vm_track.h"

namespace {

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }

__device__ __forceinline__ int wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// calcHist's uniform 8-bit lookup for 10 bins over [0, 255): 255 itself is outside
__device__ __forceinline__ int bin10(int v) { return (int)floor((double)v * (10.0 / 255.0)); }

// the bin of this lane's pixel of the patch of (x, y) in `frame`, or -1: the patch is
// cv::Range(cl(y - 3), cl(y + 3)) x cv::Range(cl(x - 3), cl(x + 3)), cl clamping into the frame
__device__ __forceinline__ int patch_bin(const uchar4 *__restrict__ frame, int w, int h, int x, int y, int lane)
{
    const int lx = clampi(x - 3, w), rx = clampi(x + 3, w), ly = clampi(y - 3, h), ry = clampi(y + 3, h);
    const int px = lx + lane % 6, py = ly + lane / 6;
    if (lane >= 36 || px >= rx || py >= ry) return -1;
    const uchar4 c = frame[(size_t)py * w + px];
    if (c.x == 255 || c.y == 255 || c.z == 255) return -1;
    return bin10(c.x) * 100 + bin10(c.y) * 10 + bin10(c.z);
}

// compareHist(h1, h2, HISTCMP_CORREL) over 1000 bins from the exact sums, fabs, as float
__device__ __forceinline__ float correl(int s1, int s11, int s2, int s22, int s12)
{
    const double scale = 1.0 / 1000;
    const double num = (double)s12 - ((double)s1 * (double)s2) * scale;
    const double den2 = ((double)s11 - ((double)s1 * (double)s1) * scale) * ((double)s22 - ((double)s2 * (double)s2) * scale);
    const double r = fabs(den2) > __DBL_EPSILON__ ? __ddiv_rn(num, __dsqrt_rn(den2)) : 1.0;
    return (float)fabs(r);
}

// pt.p.x += F.x + 0.5 on an int (UI/MdiEditor.cpp:1241-1249): F read at the clamped point, the point unclamped
__device__ __forceinline__ void flow_step(int &x, int &y, const float2 *__restrict__ fl, int w, int h)
{
    const float2 F = fl[(size_t)clampi(y, h) * w + clampi(x, w)];
    x = (int)((double)x + ((double)F.x + 0.5));
    y = (int)((double)y + ((double)F.y + 0.5));
}

// a key's histogram into hk (zero on entry); s = sum h, ss = sum h^2
__device__ void key_hist(const uchar4 *frame, int w, int h, int x, int y, int lane, int *hk, int &s, int &ss)
{
    const int bin = patch_bin(frame, w, h, x, y, lane);
    if (bin >= 0) atomicAdd(&hk[bin], 1);
    __syncthreads();
    s = wave_sum(bin >= 0);
    ss = wave_sum(bin >= 0 ? hk[bin] : 0);
    __syncthreads();
}

struct PatchSums {
    int s1, s11, s12m, s12o;
};

// the current point's patch against hm (and ho): cur is zero on entry and on return
__device__ PatchSums patch_sums(const uchar4 *frame, int w, int h, int x, int y, int lane, int *cur, const int *hm,
                                const int *ho)
{
    const int bin = patch_bin(frame, w, h, x, y, lane);
    if (bin >= 0) atomicAdd(&cur[bin], 1);
    __syncthreads();
    PatchSums r;
    r.s1 = wave_sum(bin >= 0);
    r.s11 = wave_sum(bin >= 0 ? cur[bin] : 0);
    r.s12m = wave_sum(bin >= 0 ? hm[bin] : 0);
    r.s12o = wave_sum(bin >= 0 ? ho[bin] : 0);
    __syncthreads();
    if (bin >= 0) cur[bin] = 0;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(64) void k_track(const vm_track_segment *__restrict__ segs, const uchar4 *__restrict__ video0,
                                              const uchar4 *__restrict__ video1, const float2 *__restrict__ f0,
                                              const float2 *__restrict__ f1, const float2 *__restrict__ b0,
                                              const float2 *__restrict__ b1, int w, int h, int depth,
                                              vm_track_point *__restrict__ out)
{
    __shared__ int hm[1000], ho[1000], cur[1000];
    const int lane = threadIdx.x;
    const vm_track_segment sg = segs[blockIdx.x];
    const size_t page = (size_t)w * h;
    const uchar4 *video = sg.side ? video1 : video0;
    const float2 *fw = sg.side ? f1 : f0, *bw = sg.side ? b1 : b0;
    vm_track_point *o = out + (size_t)blockIdx.x * depth;
    for (int i = lane; i < 1000; i += 64) hm[i] = ho[i] = cur[i] = 0;
    __syncthreads();
    int sm, smm;
    key_hist(video + (size_t)sg.frame * page, w, h, sg.x, sg.y, lane, hm, sm, smm);
    if (sg.ofr < 0) { // chain: AddPoint's loops, MovePoint's with no key on that side
        int x = sg.x, y = sg.y;
        for (int s = sg.frame + sg.dir; s >= 0 && s < depth; s += sg.dir) {
            flow_step(x, y, (sg.dir > 0 ? fw : bw) + (size_t)(s - sg.dir) * page, w, h);
            const PatchSums p = patch_sums(video + (size_t)s * page, w, h, x, y, lane, cur, hm, ho);
            if (lane == 0) o[s] = vm_track_point{x, y, correl(p.s1, p.s11, sm, smm, p.s12m)};
        }
        return;
    }
    // blend: c_o (from the other key towards the moved one) parks in the output slots, then c_m
    // walks from the moved key and blends with it frame by frame (UI/MdiEditor.cpp:1315-1339, 1368-1392)
    const int dir = sg.ofr > sg.frame ? 1 : -1;
    int so, soo;
    key_hist(video + (size_t)sg.ofr * page, w, h, sg.ox, sg.oy, lane, ho, so, soo);
    {
        int x = sg.ox, y = sg.oy;
        for (int s = sg.ofr - dir; s != sg.frame; s -= dir) {
            flow_step(x, y, (dir < 0 ? fw : bw) + (size_t)(s + dir) * page, w, h);
            if (lane == 0) o[s] = vm_track_point{x, y, 0.f};
        }
    }
    __syncthreads(); // the workgroup is this wave: its own stores are visible to all its lanes after the barrier
    const float span = (float)abs(sg.ofr - sg.frame);
    int x = sg.x, y = sg.y;
    for (int s = sg.frame + dir; s != sg.ofr; s += dir) {
        flow_step(x, y, (dir > 0 ? fw : bw) + (size_t)(s - dir) * page, w, h);
        const vm_track_point co = o[s];
        const float fa = (float)abs(sg.ofr - s) / span;
        const int bx = (int)((float)x * fa + (float)co.x * (1.0f - fa));
        const int by = (int)((float)y * fa + (float)co.y * (1.0f - fa));
        const PatchSums p = patch_sums(video + (size_t)s * page, w, h, bx, by, lane, cur, hm, ho);
        const float wm = correl(p.s1, p.s11, sm, smm, p.s12m), wo = correl(p.s1, p.s11, so, soo, p.s12o);
        __syncthreads(); // every lane has read o[s] before lane 0 overwrites it
        if (lane == 0) o[s] = vm_track_point{bx, by, wm * fa + wo * (1.0f - fa)};
    }
}

__global__ __launch_bounds__(256) void k_rgba(const uint8_t *__restrict__ rgb, int pitch, int w, int h, uchar4 *__restrict__ out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint8_t *p = rgb + (size_t)y * pitch + 3 * x;
    out[(size_t)y * w + x] = make_uchar4(p[0], p[1], p[2], 0);
}

} // namespace

void vm_track_launch(const vm_track_segment *seg, int n, const uchar4 *frame0, const uchar4 *frame1, const float2 *f0,
                     const float2 *f1, const float2 *b0, const float2 *b1, int w, int h, int depth, vm_track_point *out,
                     hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(k_track, dim3(n), dim3(64), 0, s, seg, frame0, frame1, f0, f1, b0, b1, w, h, depth, out);
}

void vm_track_launch_rgba(const uint8_t *rgb, int pitch, int w, int h, uchar4 *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_rgba, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, s, rgb, pitch, w, h, out);
}
