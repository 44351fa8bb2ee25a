// vm_flow.cpp -- host side of the dense optical flow (MdiEditor::OpticalFlow, UI/MdiEditor.cpp:1584-1689):
// parameter checks, the scale table, the per-call working set and the launch sequence of vm_flow.hip;
// the C-ABI entry points for independent frame pairs.  The video and sync entry points live beside
// their objects (vm_pyramid_api.cpp, vm_sync.cpp, vm_track.cpp) and call vm_flow_run_videos.
#include "vm_host.h"
#include "vm_flow.h"

#include <algorithm>
#include <cmath>

namespace {

struct Scale {
    double s;
    int w, h;
};

// s_k = pyr_scale^k for k = 0..L, L the largest k <= num_levels with w s_j >= 32 and h s_j >= 32 for all j <= k
std::vector<Scale> scale_table(int w, int h, const vm_flow_params &p)
{
    std::vector<Scale> t;
    for (int k = 0; k <= p.num_levels; ++k) {
        const double s = std::pow((double)p.pyr_scale, k);
        if (w * s < 32 || h * s < 32) break;
        t.push_back({s, (int)std::rint(w * s), (int)std::rint(h * s)});
    }
    return t;
}

std::vector<double> gauss(double sigma, int n)
{
    std::vector<double> g(2 * n + 1);
    double sum = 0;
    for (int i = -n; i <= n; ++i) sum += (g[i + n] = std::exp(-(double)i * i / (2 * sigma * sigma)));
    for (double &x : g) x /= sum;
    return g;
}

int blur_radius(double s)
{
    const double sigma = (1.0 / s - 1.0) * 0.5;
    return std::max(3, (int)std::rint(sigma * 5) | 1) / 2;
}

VmPolyConst poly_const(const vm_flow_params &p)
{
    VmPolyConst pc{};
    pc.n = p.poly_n / 2;
    const std::vector<double> g = gauss(p.poly_sigma, pc.n);
    double m0 = 0, m2 = 0, m4 = 0;
    for (int i = -pc.n; i <= pc.n; ++i) {
        const double v = g[i + pc.n];
        pc.g[i + pc.n] = (float)v;
        m0 += v;
        m2 += v * i * i;
        m4 += v * i * i * i * i;
    }
    // inverse of [[m0^2, m0 m2, m0 m2], [m0 m2, m0 m4, m2^2], [m0 m2, m2^2, m0 m4]]: rows 1 and 2 (A_xx, A_yy)
    const double G[3][3] = {{m0 * m0, m0 * m2, m0 * m2}, {m0 * m2, m0 * m4, m2 * m2}, {m0 * m2, m2 * m2, m0 * m4}};
    const double det = G[0][0] * (G[1][1] * G[2][2] - G[1][2] * G[2][1]) - G[0][1] * (G[1][0] * G[2][2] - G[1][2] * G[2][0]) +
                       G[0][2] * (G[1][0] * G[2][1] - G[1][1] * G[2][0]);
    pc.q0 = (float)((G[1][2] * G[2][0] - G[1][0] * G[2][2]) / det);
    pc.q1 = (float)((G[0][0] * G[2][2] - G[0][2] * G[2][0]) / det);
    pc.q2 = (float)((G[0][2] * G[1][0] - G[0][0] * G[1][2]) / det);
    pc.ib = (float)(1.0 / (m0 * m2));
    pc.ixy = (float)(1.0 / (m2 * m2));
    return pc;
}

} // namespace

int vm_flow_resolve(const vm_flow_params *p, int w, int h, vm_flow_params *out, const char *fn)
{
    vm_flow_params q;
    vm_flow_params_default(&q);
    if (p) q = *p;
    if (q.fast_pyramids != 0) return vm_fail(VM_E_INVALID, "%s: fast_pyramids is not supported", fn);
    if (q.flags != 0) return vm_fail(VM_E_INVALID, "%s: flags %d not supported (Gaussian window / initial flow)", fn, q.flags);
    if (q.num_levels < 0 || !(q.pyr_scale > 0.f && q.pyr_scale < 1.f) || q.win_size < 3 || q.win_size > 31 ||
        q.win_size % 2 == 0 || q.num_iters < 1 || (q.poly_n != 5 && q.poly_n != 7) || !(q.poly_sigma > 0.f) ||
        !std::isfinite(q.poly_sigma))
        return vm_fail(VM_E_INVALID, "%s: parameters out of range (num_levels >= 0, 0 < pyr_scale < 1, odd win_size 3..31, "
                                     "num_iters >= 1, poly_n 5 or 7, poly_sigma > 0)", fn);
    if (w < 32 || h < 32) return vm_fail(VM_E_INVALID, "%s: frames of %d x %d (at least 32 x 32 wanted)", fn, w, h);
    if ((double)w * h > 1e9) return vm_fail(VM_E_INVALID, "%s: frames of %d x %d are too large", fn, w, h);
    for (const Scale &sc : scale_table(w, h, q))
        if (sc.s < 1.0 && blur_radius(sc.s) > VM_FLOW_MAX_BLUR_R)
            return vm_fail(VM_E_INVALID, "%s: the scale %g needs a blur radius above %d px", fn, sc.s, VM_FLOW_MAX_BLUR_R);
    *out = q;
    return VM_OK;
}

size_t vm_flow_frame_bytes(int w, int h, const vm_flow_params &p)
{
    size_t b = 0;
    for (const Scale &sc : scale_table(w, h, p)) b += (size_t)sc.w * sc.h * 20;
    return b;
}

size_t vm_flow_flow_bytes(int w, int h) { return (size_t)w * h * 24; }

// the frames per chunk of a video walk (F frames of each of `videos` videos, 2 (F - 1) flows each)
static int vm_flow_video_chunk(int w, int h, const vm_flow_params &p, int videos)
{
    // F frames of each video: videos * (F frame_bytes + 2 (F - 1) flow_bytes) <= budget
    const double per = (double)videos * ((double)vm_flow_frame_bytes(w, h, p) + 2.0 * vm_flow_flow_bytes(w, h));
    return std::max(2, (int)std::min(1e6, (double)VM_FLOW_BUDGET / per));
}

int vm_flow_run(vm_ctx *c, int w, int h, const vm_flow_params &p, int nframes, const VmFlowSource &src,
                const std::vector<VmFlowPair> &pairs)
{
    hipStream_t s = c->stream;
    const std::vector<Scale> sc = scale_table(w, h, p);
    const int L = (int)sc.size();
    const size_t n0 = (size_t)w * h;
    const int nf = (int)pairs.size();
    // blur taps of every scale k > 0, concatenated
    std::vector<float> taps;
    std::vector<size_t> tap_off(L, 0);
    for (int k = 1; k < L; ++k) {
        const int r = blur_radius(sc[k].s);
        tap_off[k] = taps.size();
        for (double g : gauss((1.0 / sc[k].s - 1.0) * 0.5, r)) taps.push_back((float)g);
    }
    std::vector<size_t> off(L, 0); // scale k's planes start at off[k] (elements of p0 / p1), nframes planes each
    size_t tot = 0;
    for (int k = 0; k < L; ++k) {
        off[k] = tot;
        tot += (size_t)nframes * sc[k].w * sc[k].h;
    }
    VmDev<float> grey, tmp, blurred, img, dtaps;
    VmDev<float4> p0;
    VmDev<float> p1;
    VmDev<float2> d[2];
    VmDev<int2> dpairs;
    if (int rc = grey.reserve(n0)) return rc;
    if (int rc = tmp.reserve(n0)) return rc;
    if (int rc = blurred.reserve(n0)) return rc;
    if (int rc = img.reserve(n0)) return rc;
    if (int rc = dtaps.reserve(std::max<size_t>(taps.size(), 1))) return rc;
    if (int rc = p0.reserve(tot)) return rc;
    if (int rc = p1.reserve(tot)) return rc;
    if (nf > 0) {
        for (auto &b : d)
            if (int rc = b.reserve(n0 * nf)) return rc;
        if (int rc = dpairs.reserve(nf)) return rc;
    }
    if (!taps.empty()) VM_HIP(hipMemcpyAsync(dtaps.get(), taps.data(), taps.size() * 4, hipMemcpyHostToDevice, s));
    const VmPolyConst pc = poly_const(p);
    // per frame, once: grey, scale images, polynomial expansion of each scale
    for (int i = 0; i < nframes; ++i) {
        if (int rc = src(i, grey.get())) return rc;
        for (int k = 0; k < L; ++k) {
            const float *im = grey.get();
            if (k > 0) {
                vm_flow_launch_blur(grey.get(), tmp.get(), blurred.get(), w, h, dtaps.get() + tap_off[k], blur_radius(sc[k].s), s);
                vm_flow_launch_resize(blurred.get(), w, h, img.get(), sc[k].w, sc[k].h, s);
                im = img.get();
            }
            const size_t o = off[k] + (size_t)i * sc[k].w * sc[k].h;
            vm_flow_launch_poly(im, sc[k].w, sc[k].h, pc, p0.get() + o, p1.get() + o, s);
        }
        VM_HIP(hipGetLastError());
    }
    if (nf > 0) {
        std::vector<int2> hp(nf);
        for (int f = 0; f < nf; ++f) hp[f] = make_int2(pairs[f].a, pairs[f].b);
        VM_HIP(hipMemcpyAsync(dpairs.get(), hp.data(), nf * sizeof(int2), hipMemcpyHostToDevice, s));
        int cur = 0;
        for (int k = L - 1; k >= 0; --k) {
            const size_t plane = (size_t)sc[k].w * sc[k].h;
            if (k == L - 1) VM_HIP(hipMemsetAsync(d[cur].get(), 0, plane * nf * sizeof(float2), s));
            for (int it = 0; it < p.num_iters; ++it) {
                vm_flow_launch_iter(p0.get() + off[k], p1.get() + off[k], plane, dpairs.get(), nf, d[cur].get(), d[cur ^ 1].get(),
                                    sc[k].w, sc[k].h, p.win_size, s);
                cur ^= 1;
            }
            if (k > 0) {
                vm_flow_launch_resize_flow(d[cur].get(), sc[k].w, sc[k].h, d[cur ^ 1].get(), sc[k - 1].w, sc[k - 1].h,
                                           1.f / p.pyr_scale, nf, s);
                cur ^= 1;
            }
            VM_HIP(hipGetLastError());
        }
        for (int f = 0; f < nf; ++f)
            VM_HIP(hipMemcpyAsync(pairs[f].out, d[cur].get() + (size_t)f * n0, n0 * sizeof(float2), hipMemcpyDeviceToDevice, s));
    }
    VM_HIP(hipStreamSynchronize(s)); // the working set is freed on return
    return VM_OK;
}

int vm_flow_run_videos(vm_ctx *c, int w, int h, int d, const vm_flow_params &p, const VmFlowVideoSource &src,
                       const VmFlowVideoOut &fwd, const VmFlowVideoOut &bwd)
{
    const int F = vm_flow_video_chunk(w, h, p, 2);
    for (int t0 = 0; t0 < d - 1; t0 += F - 1) {
        const int t1 = std::min(d - 1, t0 + F - 1), nfr = t1 - t0 + 1;
        std::vector<VmFlowPair> pairs;
        for (int k = 0; k < 2; ++k)
            for (int t = t0; t <= t1; ++t) { // frame slot of (video k, frame t): k * nfr + t - t0
                const int slot = k * nfr + t - t0;
                if (t < t1) pairs.push_back({slot, slot + 1, fwd(k, t)});
                if (bwd && t > t0) pairs.push_back({slot, slot - 1, bwd(k, t)});
            }
        auto chunk = [&](int f, float *dst) -> int { return src(f / nfr, t0 + f % nfr, dst); };
        if (int rc = vm_flow_run(c, w, h, p, 2 * nfr, chunk, pairs)) return rc;
    }
    return VM_OK;
}

extern "C" int vm_flow_params_default(vm_flow_params *p)
{
    if (!p) return vm_fail(VM_E_INVALID, "vm_flow_params_default: NULL argument");
    p->num_levels = 5;
    p->pyr_scale = 0.5f;
    p->fast_pyramids = 0;
    p->win_size = 13;
    p->num_iters = 10;
    p->poly_n = 5;
    p->poly_sigma = 1.1f;
    p->flags = 0;
    return VM_OK;
}

// n independent pairs: frames 2i / 2i + 1 of a chunk are a[i] / b[i]
static int optical_flow_pairs(vm_ctx *ctx, int w, int h, int n, const void *const *a, const void *const *b, int rgb, int pitch,
                              const vm_flow_params *pp, float *const *flow_xy, const char *fn)
{
    if (!ctx) return vm_fail(VM_E_INVALID, "%s: null handle", fn);
    if (n < 0 || (n > 0 && (!a || !b || !flow_xy))) return vm_fail(VM_E_INVALID, "%s: bad arguments", fn);
    vm_flow_params p;
    if (int rc = vm_flow_resolve(pp, w, h, &p, fn)) return rc;
    const size_t unit = rgb ? 1 : 4, row = rgb ? (size_t)3 * w : (size_t)4 * w; // pitch in bytes (RGB) or floats (luma)
    if (int rc = vm_pitch_resolve(fn, &pitch, unit, row)) return rc;
    for (int i = 0; i < n; ++i)
        if (!a[i] || !b[i] || !flow_xy[i]) return vm_fail(VM_E_INVALID, "%s: pair %d has a NULL array", fn, i);
    if (!vm_ctx_alive(ctx)) return vm_fail(VM_E_INVALID, "%s: the context was destroyed", fn);
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    VM_ON_DEVICE(ctx);
    hipStream_t s = ctx->stream;
    const size_t n0 = (size_t)w * h;
    const int per = std::max(1, (int)std::min<double>(n, (double)VM_FLOW_BUDGET /
                                                             (2.0 * vm_flow_frame_bytes(w, h, p) + vm_flow_flow_bytes(w, h))));
    VmDev<uint8_t> stage;
    VmDev<float2> out;
    if (int rc = stage.reserve(rgb ? n0 * 3 : 1)) return rc;
    if (int rc = out.reserve(n0 * std::max(1, std::min(per, n)))) return rc;
    for (int i0 = 0; i0 < n; i0 += per) {
        const int m = std::min(per, n - i0);
        std::vector<VmFlowPair> pairs(m);
        for (int j = 0; j < m; ++j) pairs[j] = {2 * j, 2 * j + 1, out.get() + (size_t)j * n0};
        auto src = [&](int f, float *dst) -> int {
            const void *hs = (f & 1 ? b : a)[i0 + f / 2];
            if (int rc = vm_copy_pitched(fn, hipMemcpyHostToDevice, rgb ? (void *)stage.get() : (void *)dst, row, hs, pitch, unit, row, h, s)) return rc;
            if (rgb) vm_flow_launch_grey_rgb(stage.get(), w * 3, w, h, dst, s);
            return VM_OK;
        };
        if (int rc = vm_flow_run(ctx, w, h, p, 2 * m, src, pairs)) return rc;
        for (int j = 0; j < m; ++j)
            VM_HIP(hipMemcpyAsync(flow_xy[i0 + j], out.get() + (size_t)j * n0, n0 * sizeof(float2), hipMemcpyDeviceToHost, s));
        VM_HIP(hipStreamSynchronize(s));
    }
    return VM_OK;
}

extern "C" int vm_optical_flow_rgb(vm_ctx *ctx, int w, int h, int n, const uint8_t *const *a, const uint8_t *const *b,
                                   int pitch_bytes, const vm_flow_params *p, float *const *flow_xy)
{
    return optical_flow_pairs(ctx, w, h, n, (const void *const *)a, (const void *const *)b, 1, pitch_bytes, p, flow_xy,
                              "vm_optical_flow_rgb");
}

extern "C" int vm_optical_flow_luma(vm_ctx *ctx, int w, int h, int n, const float *const *a, const float *const *b,
                                    int pitch, const vm_flow_params *p, float *const *flow_xy)
{
    return optical_flow_pairs(ctx, w, h, n, (const void *const *)a, (const void *const *)b, 0, pitch, p, flow_xy,
                              "vm_optical_flow_luma");
}
