// vm_flow.hip -- dense optical flow for gfx950: Farneback's two-frame polynomial-expansion method
// (spec in tests/flow_ref.py), the flow MdiEditor::OpticalFlow computes with
// cuda::FarnebackOpticalFlow before every pyramid build (UI/MdiEditor.cpp:1584-1689).
//
// Per frame (once, shared by every flow that uses the frame): grey, the scale images (separable
// Gaussian of the full-resolution frame through LDS row / column tiles, then a bilinear resize),
// and the polynomial expansion of each scale (one LDS tile: three vertical filters, six horizontal
// combinations, the constant inverse Gram matrix) into two planes, float4 (b_x, b_y, A_xx, A_yy)
// and float A_xy.
//
// Per flow, per scale, per iteration: ONE launch for all flows of a call (blockIdx.z = flow).  A
// workgroup computes the five values of A'A and A'db for its 32 x TH tile plus a win/2 halo into
// LDS, box-sums them there separably (rows into registers, back into the same LDS, then columns),
// solves the 2 x 2 system and writes d.  The five intermediate planes never reach HBM.  HBM traffic
// per pixel: d in (8 B), the a side's planes (20 B), the b side's planes gathered at x + d (20 B
// plus what the bilinear footprint misses in cache), d out (8 B).
//
// Every sum has a fixed order, there are no atomics: a flow's bits do not depend on its batch.
#include "vm_flow.h"

namespace {

__device__ __forceinline__ int reflect101(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1); // one reflection suffices (radius < n); the clamp keeps any read in bounds
}

__global__ __launch_bounds__(256) void k_grey_rgb(const uint8_t *__restrict__ rgb, int pitch, int w, int h,
                                                  float *__restrict__ out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint8_t *p = rgb + (size_t)y * pitch + 3 * x;
    const int g = (4899 * (int)p[0] + 9617 * (int)p[1] + 1868 * (int)p[2] + 8192) >> 14;
    out[(size_t)y * w + x] = (float)g;
}

__global__ __launch_bounds__(256) void k_grey_rgba(const uchar4 *__restrict__ rgba, int w, int h, float *__restrict__ out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const uchar4 c = rgba[(size_t)y * w + x];
    const int g = (4899 * (int)c.x + 9617 * (int)c.y + 1868 * (int)c.z + 8192) >> 14;
    out[(size_t)y * w + x] = (float)g;
}

// rows: 256 outputs of one row per workgroup, the row segment plus its r-halo in LDS
__global__ __launch_bounds__(256) void k_blur_rows(const float *__restrict__ src, float *__restrict__ dst, int w, int h,
                                                   const float *__restrict__ taps, int r)
{
    extern __shared__ float lds[];
    float *line = lds, *tp = lds + 256 + 2 * r;
    const int y = blockIdx.y, x0 = blockIdx.x * 256;
    const float *row = src + (size_t)y * w;
    for (int i = threadIdx.x; i < 256 + 2 * r; i += 256) line[i] = row[reflect101(x0 + i - r, w)];
    for (int i = threadIdx.x; i <= 2 * r; i += 256) tp[i] = taps[i];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    float acc = 0.f;
    for (int j = 0; j <= 2 * r; ++j) acc += tp[j] * line[threadIdx.x + j];
    dst[(size_t)y * w + x] = acc;
}

// columns: a 64-wide, 64-tall output tile per workgroup (64 x 4 threads), its rows plus the r-halo in LDS
#define VM_BLUR_CT 64
__global__ __launch_bounds__(256) void k_blur_cols(const float *__restrict__ src, float *__restrict__ dst, int w, int h,
                                                   const float *__restrict__ taps, int r)
{
    extern __shared__ float lds[];
    const int nrow = VM_BLUR_CT + 2 * r;
    float *tile = lds, *tp = lds + (size_t)nrow * 64;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * VM_BLUR_CT, tx = threadIdx.x, ty = threadIdx.y;
    const int x = min(x0 + tx, w - 1);
    for (int i = ty; i < nrow; i += 4) tile[i * 64 + tx] = src[(size_t)reflect101(y0 + i - r, h) * w + x];
    for (int i = ty * 64 + tx; i <= 2 * r; i += 256) tp[i] = taps[i];
    __syncthreads();
    if (x0 + tx >= w) return;
    for (int o = ty; o < VM_BLUR_CT; o += 4) {
        const int y = y0 + o;
        if (y >= h) break;
        float acc = 0.f;
        for (int j = 0; j <= 2 * r; ++j) acc += tp[j] * tile[(o + j) * 64 + tx];
        dst[(size_t)y * w + x0 + tx] = acc;
    }
}

struct Axis {
    int i0, i1;
    float f;
};
__device__ __forceinline__ Axis axis(int x, int n_src, int n_dst)
{
    float s = ((float)x + 0.5f) * (float)n_src / (float)n_dst - 0.5f;
    s = fminf(fmaxf(s, 0.f), (float)(n_src - 1));
    Axis a;
    a.i0 = min((int)floorf(s), n_src - 1);
    a.i1 = min(a.i0 + 1, n_src - 1);
    a.f = s - (float)a.i0;
    return a;
}

__global__ __launch_bounds__(256) void k_resize(const float *__restrict__ src, int W, int H, float *__restrict__ dst,
                                                int w, int h)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const Axis ax = axis(x, W, w), ay = axis(y, H, h);
    const float *r0 = src + (size_t)ay.i0 * W, *r1 = src + (size_t)ay.i1 * W;
    const float top = r0[ax.i0] * (1.f - ax.f) + r0[ax.i1] * ax.f;
    const float bot = r1[ax.i0] * (1.f - ax.f) + r1[ax.i1] * ax.f;
    dst[(size_t)y * w + x] = top * (1.f - ay.f) + bot * ay.f;
}

__global__ __launch_bounds__(256) void k_resize_flow(const float2 *__restrict__ src, int W, int H, float2 *__restrict__ dst,
                                                     int w, int h, float mul)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    src += (size_t)blockIdx.z * W * H;
    dst += (size_t)blockIdx.z * w * h;
    const Axis ax = axis(x, W, w), ay = axis(y, H, h);
    const float2 *r0 = src + (size_t)ay.i0 * W, *r1 = src + (size_t)ay.i1 * W;
    const float2 a = r0[ax.i0], b = r0[ax.i1], c = r1[ax.i0], d = r1[ax.i1];
    const float tx = a.x * (1.f - ax.f) + b.x * ax.f, bx = c.x * (1.f - ax.f) + d.x * ax.f;
    const float ty = a.y * (1.f - ax.f) + b.y * ax.f, by = c.y * (1.f - ax.f) + d.y * ax.f;
    dst[(size_t)y * w + x] = make_float2((tx * (1.f - ay.f) + bx * ay.f) * mul, (ty * (1.f - ay.f) + by * ay.f) * mul);
}

// polynomial expansion: a 32 x 16 output tile per workgroup (32 x 8 threads), replicate border
#define VM_PX 32
#define VM_PY 16
__global__ __launch_bounds__(256) void k_poly(const float *__restrict__ img, int w, int h, VmPolyConst pc,
                                              float4 *__restrict__ p0, float *__restrict__ p1)
{
    constexpr int NW = VM_PX + 6, NH = VM_PY + 6;
    __shared__ float t_img[NH][NW];
    __shared__ float t_v[3][VM_PY][NW];
    const int n = pc.n, x0 = blockIdx.x * VM_PX, y0 = blockIdx.y * VM_PY;
    const int tid = threadIdx.y * VM_PX + threadIdx.x;
    const int nw = VM_PX + 2 * n, nh = VM_PY + 2 * n;
    for (int i = tid; i < nw * nh; i += 256) {
        const int r = i / nw, c = i % nw;
        const int yy = min(max(y0 + r - n, 0), h - 1), xx = min(max(x0 + c - n, 0), w - 1);
        t_img[r][c] = img[(size_t)yy * w + xx];
    }
    __syncthreads();
    for (int i = tid; i < VM_PY * nw; i += 256) {
        const int r = i / nw, c = i % nw;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        for (int j = 0; j <= 2 * n; ++j) {
            const float t = (float)(j - n), f = pc.g[j] * t_img[r + j][c];
            v0 += f;
            v1 += t * f;
            v2 += t * t * f;
        }
        t_v[0][r][c] = v0;
        t_v[1][r][c] = v1;
        t_v[2][r][c] = v2;
    }
    __syncthreads();
    const int tx = threadIdx.x, x = x0 + tx;
    for (int r = threadIdx.y; r < VM_PY; r += 8) {
        const int y = y0 + r;
        if (x >= w || y >= h) continue;
        float s1 = 0.f, sx = 0.f, sxx = 0.f, sy = 0.f, sxy = 0.f, syy = 0.f;
        for (int j = 0; j <= 2 * n; ++j) {
            const float t = (float)(j - n), g = pc.g[j];
            const float a = t_v[0][r][tx + j], b = t_v[1][r][tx + j], c = t_v[2][r][tx + j];
            s1 += g * a;
            sx += g * t * a;
            sxx += g * t * t * a;
            sy += g * b;
            sxy += g * t * b;
            syy += g * c;
        }
        const size_t p = (size_t)y * w + x;
        p0[p] = make_float4(sx * pc.ib, sy * pc.ib, pc.q0 * s1 + pc.q1 * sxx + pc.q2 * syy, pc.q0 * s1 + pc.q2 * sxx + pc.q1 * syy);
        p1[p] = sxy * pc.ixy;
    }
}

__device__ __forceinline__ float edge_weight(int i, int n)
{
    const int d = min(i, n - 1 - i);
    return d < 2 ? 0.14f : d < 5 ? 0.4472f : 1.f;
}

// one iteration: tile 32 x TH (TH = 32 for win <= 17, else 16), 32 x 8 threads; LDS = 5 (TH + 2R) (32 + 2R) floats
#define VM_IT_W 32
#define VM_IT_HMAX 6 // row-pass items per thread: (TH + 2R) * 32 <= 6 * 256 for both tile heights
__global__ __launch_bounds__(256) void k_iter(const float4 *__restrict__ p0, const float *__restrict__ p1, size_t plane,
                                              const int2 *__restrict__ pairs, const float2 *__restrict__ d_in,
                                              float2 *__restrict__ d_out, int w, int h, int R, int TH)
{
    extern __shared__ float lds[];
    const int NW = VM_IT_W + 2 * R, NH = TH + 2 * R, NC = NW * NH;
    const int tid = threadIdx.y * 32 + threadIdx.x;
    const int x0 = blockIdx.x * VM_IT_W, y0 = blockIdx.y * TH;
    const int2 pr = pairs[blockIdx.z];
    const float4 *pa0 = p0 + (size_t)pr.x * plane, *pb0 = p0 + (size_t)pr.y * plane;
    const float *pa1 = p1 + (size_t)pr.x * plane, *pb1 = p1 + (size_t)pr.y * plane;
    d_in += (size_t)blockIdx.z * plane;
    d_out += (size_t)blockIdx.z * plane;

    // 1. the five values at every tile + halo pixel (replicate border: the value of the clamped pixel)
    for (int i = tid; i < NC; i += 256) {
        const int r = i / NW, c = i % NW;
        const int py = min(max(y0 + r - R, 0), h - 1), px = min(max(x0 + c - R, 0), w - 1);
        const size_t p = (size_t)py * w + px;
        const float2 d = d_in[p];
        const float4 a0 = pa0[p];
        const float a12h = pa1[p] * 0.5f;
        float A11 = a0.z, A22 = a0.w, A12 = a12h, db1 = 0.f, db2 = 0.f;
        const float fx = (float)px + d.x, fy = (float)py + d.y;
        const float fx0 = floorf(fx), fy0 = floorf(fy);
        if (fx0 >= 0.f && fy0 >= 0.f && fx0 < (float)(w - 1) && fy0 < (float)(h - 1)) {
            const int ix = (int)fx0, iy = (int)fy0;
            const float ax = fx - fx0, ay = fy - fy0;
            const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
            const size_t q = (size_t)iy * w + ix;
            const float4 b00 = pb0[q], b01 = pb0[q + 1], b10 = pb0[q + w], b11 = pb0[q + w + 1];
            const float c00 = pb1[q], c01 = pb1[q + 1], c10 = pb1[q + w], c11 = pb1[q + w + 1];
            const float bx = w00 * b00.x + w01 * b01.x + w10 * b10.x + w11 * b11.x;
            const float by = w00 * b00.y + w01 * b01.y + w10 * b10.y + w11 * b11.y;
            const float bxx = w00 * b00.z + w01 * b01.z + w10 * b10.z + w11 * b11.z;
            const float byy = w00 * b00.w + w01 * b01.w + w10 * b10.w + w11 * b11.w;
            const float bxy = w00 * c00 + w01 * c01 + w10 * c10 + w11 * c11;
            A11 = (a0.z + bxx) * 0.5f;
            A22 = (a0.w + byy) * 0.5f;
            A12 = (a12h + bxy * 0.5f) * 0.5f;
            db1 = -(bx - a0.x) * 0.5f;
            db2 = -(by - a0.y) * 0.5f;
        }
        db1 += A11 * d.x + A12 * d.y;
        db2 += A12 * d.x + A22 * d.y;
        const float s = edge_weight(px, w) * edge_weight(py, h);
        A11 *= s; A22 *= s; A12 *= s; db1 *= s; db2 *= s;
        lds[0 * NC + i] = A11 * A11 + A12 * A12;
        lds[1 * NC + i] = A12 * (A11 + A22);
        lds[2 * NC + i] = A12 * A12 + A22 * A22;
        lds[3 * NC + i] = A11 * db1 + A12 * db2;
        lds[4 * NC + i] = A12 * db1 + A22 * db2;
    }
    __syncthreads();
    // 2. row sums over 2R + 1 for the 32 output columns of every row, into registers, then back to LDS
    const int NHW = NH * VM_IT_W;
    float hs[VM_IT_HMAX][5];
#pragma unroll
    for (int k = 0; k < VM_IT_HMAX; ++k) {
        const int i = tid + k * 256;
        if (i < NHW) {
            const int r = i / VM_IT_W, c = i % VM_IT_W;
#pragma unroll
            for (int v = 0; v < 5; ++v) {
                const float *row = lds + v * NC + r * NW + c;
                float acc = 0.f;
                for (int j = 0; j <= 2 * R; ++j) acc += row[j];
                hs[k][v] = acc;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < VM_IT_HMAX; ++k) {
        const int i = tid + k * 256;
        if (i < NHW)
#pragma unroll
            for (int v = 0; v < 5; ++v) lds[v * NHW + i] = hs[k][v];
    }
    __syncthreads();
    // 3. column sums, mean, solve
    const float inv = 1.f / (float)((2 * R + 1) * (2 * R + 1));
    const int c = threadIdx.x, x = x0 + c;
    for (int r = threadIdx.y; r < TH; r += 8) {
        const int y = y0 + r;
        if (x >= w || y >= h) continue;
        float g[5];
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            const float *col = lds + v * NHW + r * VM_IT_W + c;
            float acc = 0.f;
            for (int j = 0; j <= 2 * R; ++j) acc += col[j * VM_IT_W];
            g[v] = acc * inv;
        }
        const float idet = 1.f / (g[0] * g[2] - g[1] * g[1] + 1e-3f);
        d_out[(size_t)y * w + x] = make_float2((g[2] * g[3] - g[1] * g[4]) * idet, (g[0] * g[4] - g[1] * g[3]) * idet);
    }
}

} // namespace

void vm_flow_launch_grey_rgb(const uint8_t *rgb, int pitch_bytes, int w, int h, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_grey_rgb, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, s, rgb, pitch_bytes, w, h, out);
}
void vm_flow_launch_grey_rgba(const uchar4 *rgba, int w, int h, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_grey_rgba, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, s, rgba, w, h, out);
}
void vm_flow_launch_blur(const float *src, float *tmp, float *dst, int w, int h, const float *taps, int r, hipStream_t s)
{
    hipLaunchKernelGGL(k_blur_rows, dim3((w + 255) / 256, h), dim3(256), (size_t)(256 + 4 * r + 1) * 4, s, src, tmp, w, h, taps, r);
    hipLaunchKernelGGL(k_blur_cols, dim3((w + 63) / 64, (h + VM_BLUR_CT - 1) / VM_BLUR_CT), dim3(64, 4),
                       ((size_t)(VM_BLUR_CT + 2 * r) * 64 + 2 * r + 1) * 4, s, tmp, dst, w, h, taps, r);
}
void vm_flow_launch_resize(const float *src, int W, int H, float *dst, int w, int h, hipStream_t s)
{
    hipLaunchKernelGGL(k_resize, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, s, src, W, H, dst, w, h);
}
void vm_flow_launch_poly(const float *img, int w, int h, const VmPolyConst &pc, float4 *p0, float *p1, hipStream_t s)
{
    hipLaunchKernelGGL(k_poly, dim3((w + VM_PX - 1) / VM_PX, (h + VM_PY - 1) / VM_PY), dim3(VM_PX, 8), 0, s, img, w, h, pc, p0, p1);
}
void vm_flow_launch_iter(const float4 *p0, const float *p1, size_t plane, const int2 *pairs, int nflows,
                         const float2 *d_in, float2 *d_out, int w, int h, int win, hipStream_t s)
{
    const int R = win / 2, TH = R <= 8 ? 32 : 16;
    const size_t lds = (size_t)5 * (TH + 2 * R) * (VM_IT_W + 2 * R) * 4;
    hipLaunchKernelGGL(k_iter, dim3((w + VM_IT_W - 1) / VM_IT_W, (h + TH - 1) / TH, nflows), dim3(32, 8), lds, s, p0, p1, plane,
                       pairs, d_in, d_out, w, h, R, TH);
}
void vm_flow_launch_resize_flow(const float2 *src, int W, int H, float2 *dst, int w, int h, float mul, int nflows,
                                hipStream_t s)
{
    hipLaunchKernelGGL(k_resize_flow, dim3((w + 63) / 64, (h + 3) / 4, nflows), dim3(64, 4), 0, s, src, W, H, dst, w, h, mul);
}
