// vmorph/render.hpp -- C++ host mirror of the compositor entry points:
// render_halfway_image (UI/RenderWidget.h:52-57, Algorithm/render.cu:62-96) and
// CPoissonExt (Algorithm/PoissonExt.h), reference repository, on device-resident
// frames.
#ifndef VMORPH_RENDER_HPP
#define VMORPH_RENDER_HPP

#include <cmath>

#include "pyramid.hpp"

namespace vmorph {

// extended RGBA8 canvas of Pyramid::build, pyramid.cu:186-200
inline std::vector<unsigned char> make_extended(const unsigned char *rgb, int w, int h, int ex)
{
    int cw = w + 2 * ex, ch = h + 2 * ex;
    std::vector<unsigned char> can((size_t)cw * ch * 4, 255);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            unsigned char *d = &can[((size_t)(y + ex) * cw + x + ex) * 4];
            const unsigned char *s = &rgb[((size_t)y * w + x) * 3];
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = 0;
        }
    return can;
}

// A viewport of the morph (vm_viewport): where an out_w x out_h grid lies over the halfway domain, in pixel-EDGE
// coordinates (field pixel i covers [i, i + 1)), and how many sub-samples every output pixel takes.  The constructors
// compute in double and round once, as the Python facade's do.
struct Viewport : vm_viewport {
    Viewport(double x0_, double y0_, double step_x_, double step_y_, int out_w_, int out_h_, int nx_ = 1, int ny_ = 1)
        : vm_viewport{(float)x0_, (float)y0_, (float)step_x_, (float)step_y_, out_w_, out_h_, nx_, ny_} {}
    // the frame itself: the bits of render_halfway_image
    static Viewport identity(int w, int h) { return Viewport(0.0, 0.0, 1.0, 1.0, w, h); }
    // a w x h window at native scale with its corner at (x, y)
    static Viewport crop(double x, double y, int w, int h) { return Viewport(x, y, 1.0, 1.0, w, h); }
    // the whole w x h frame at another size
    static Viewport fit(int w, int h, int out_w, int out_h) { return Viewport(0.0, 0.0, (double)w / out_w, (double)h / out_h, out_w, out_h); }
    // an out_w x out_h window centred on (cx, cy), `factor` times enlarged
    static Viewport zoom(double cx, double cy, double factor, int out_w, int out_h)
    {
        const double step = 1.0 / factor;
        return Viewport(cx - 0.5 * out_w * step, cy - 0.5 * out_h * step, step, step, out_w, out_h);
    }
    // the w x h frame and `margin` pixels beyond every edge
    static Viewport overscan(int w, int h, int margin) { return Viewport(-(double)margin, -(double)margin, 1.0, 1.0, w + 2 * margin, h + 2 * margin); }
    // the same viewport with nx x ny sub-samples per output pixel (ny 0: nx)
    Viewport supersampled(int nx_, int ny_ = 0) const
    {
        Viewport v = *this;
        v.nx = nx_; v.ny = ny_ ? ny_ : nx_;
        return v;
    }
};

// the filter of the last taps of a filtered viewport call (VM_FILTER_*): the taps that read a canvas or a layer
enum class Filter : int {
    Bilinear = VM_FILTER_BILINEAR,          // the viewport call itself
    CatmullRom = VM_FILTER_CATMULL_ROM,     // B = 0, C = 1/2: interpolating
    Mitchell = VM_FILTER_MITCHELL,          // B = 1/3, C = 1/3
    BSpline = VM_FILTER_BSPLINE             // B = 1, C = 0: never overshoots, blurs
};

// the band table of a multiband call (vm_bands): `levels` reductions, one sharpening factor >= 1 per band, band 0 the
// finest, band `levels` the low-pass residual.  The tables are the Python facade's: computed in double, rounded once
struct Bands : vm_bands {
    // the Burt-Adelson spline: every band crosses over with the weight plane of its level as it is
    static Bands linear(int levels_)
    {
        Bands b{};
        b.levels = levels_;
        for (int l = 0; l <= VM_MULTIBAND_MAX_LEVELS; ++l) b.sharp[l] = 1.0f;
        return b;
    }
    // detail switches quickly, colour dissolves slowly: finest ^ ((levels - l) / levels) on band l, 1 on the residual
    static Bands sharpen(int levels_, double finest)
    {
        Bands b = linear(levels_);
        for (int l = 0; l < levels_ && l <= VM_MULTIBAND_MAX_LEVELS; ++l)
            b.sharp[l] = (float)std::pow(finest, (double)(levels_ - l) / levels_);
        return b;
    }
    // the deepest linear table, of at most `most` levels, whose coarsest level of a w x h frame is still at least 2 x 2
    // (0 levels for a frame too small to have one: the library refuses it)
    static Bands for_size(int w, int h, int most = 5)
    {
        int levels_ = 0;
        while (levels_ < most && levels_ < VM_MULTIBAND_MAX_LEVELS && (w + 1) / 2 >= 2 && (h + 1) / 2 >= 2) {
            w = (w + 1) / 2; h = (h + 1) / 2;
            ++levels_;
        }
        return linear(levels_);
    }
};

class Frame {
public:
    Frame(Context &ctx, int w, int h, int ex) : w_(w), h_(h), ex_(ex) { check(vm_frame_create(ctx.handle(), w, h, ex, &f_)); }
    ~Frame() { vm_frame_destroy(f_); }
    Frame(const Frame &) = delete;
    Frame &operator=(const Frame &) = delete;

    void upload(const unsigned char *ext0, const unsigned char *ext1, const float *v, const float *qpath)
    {
        check(vm_frame_upload(f_, ext0, ext1, v, qpath));
    }
    // the canvases built on the device from the two RGB8 frames (Pyramid::build, pyramid.cu:186-200)
    void upload_rgb(const unsigned char *rgb0, const unsigned char *rgb1, int pitch_bytes = 0) { check(vm_frame_upload_rgb(f_, rgb0, rgb1, pitch_bytes)); }
    void set_v_from_level(Pyramid &pyr, int el) { check(vm_frame_set_v_from_level(f_, pyr.handle(), el - 1)); }

    // CPoissonExt::run body for one side, PoissonExt.cpp:19-41
    int poisson_extend(int side, float tol = 1e-5f, int max_it = 20000)
    {
        int it = 0;
        check(vm_poisson_extend(f_, side, tol, max_it, &it, nullptr, nullptr));
        return it;
    }
    // CQuadraticPath::optimize for this frame (QuadraticPath.cpp:24-223): u stays in the frame
    int quadratic_path(float tol = 1e-4f, int max_it = 200)
    {
        int it = 0;
        check(vm_frame_quadratic_path(f_, tol, max_it, &it, nullptr, nullptr));
        return it;
    }
    std::vector<float> download_qpath()
    {
        std::vector<float> out((size_t)w_ * h_ * 2);
        check(vm_frame_download_qpath(f_, out.data()));
        return out;
    }
    std::vector<unsigned char> download_ext(int side)
    {
        std::vector<unsigned char> out((size_t)(w_ + 2 * ex_) * (h_ + 2 * ex_) * 4);
        check(vm_frame_download_ext(f_, side, out.data()));
        return out;
    }
    // render_halfway_image(out, rowstride, w, h, ex, color_fa, geo_fa, color_from, ...)
    std::vector<unsigned char> render_halfway_image(float color_fa, float geo_fa, int color_from)
    { return rendered<unsigned char>(rgb_bytes(), vm_render_halfway, color_fa, geo_fa, color_from); }

    // where every output pixel of render_halfway_image at geo_fa samples image 0 and image 1 (vm_frame_sampling_maps):
    // the renderer's fixed point (render.cu:16-60) with its two positions kept
    struct SamplingMaps {
        std::vector<float> map0, map1;      // (h, w, 2): image pixels, pixel centre i is i
        std::vector<float> resid;           // (h, w): the move of the last round
        std::vector<unsigned char> flags;   // (h, w): bit 0 / 1: map0 / map1 inside the image
    };
    SamplingMaps sampling_maps(float geo_fa)
    {
        const size_t n = (size_t)w_ * h_;
        SamplingMaps m{std::vector<float>(2 * n), std::vector<float>(2 * n), std::vector<float>(n), std::vector<unsigned char>(n)};
        check(vm_frame_sampling_maps(f_, geo_fa, m.map0.data(), m.map1.data(), m.resid.data(), m.flags.data()));
        return m;
    }
    // two (h, w, channels) float layers, channels in 1..4, kept on the device for render_layers
    void upload_layers(int channels, const float *layer0, const float *layer1, int pitch_floats = 0)
    {
        check(vm_frame_upload_layers(f_, channels, layer0, layer1, pitch_floats));
        channels_ = channels;
    }
    // the layers extended past the image edge as the canvases are (vm_frame_extend_layers; PoissonExt.cpp:49-362): from then
    // on every layer render call samples the extension instead of repeating the edge texel; a new upload_layers drops it.
    // Returns the iterations of every system: side 1 then side 2 per group of up to three channels
    std::vector<int> extend_layers(float tol = 1e-5f, int max_it = 20000)
    {
        std::vector<int> it(2 * ((channels_ + 2) / 3 > 0 ? (channels_ + 2) / 3 : 1), 0);
        check(vm_frame_extend_layers(f_, tol, max_it, it.data(), nullptr, nullptr));
        return it;
    }
    // the extended layer of side 1 or 2: (h + 2 ex, w + 2 ex, channels) floats
    std::vector<float> download_layers_ext(int side)
    {
        std::vector<float> out((size_t)(w_ + 2 * ex_) * (h_ + 2 * ex_) * (channels_ > 0 ? channels_ : 1));
        check(vm_frame_download_layers_ext(f_, side, out.data(), 0));
        return out;
    }
    // back to the tight layers
    void drop_layer_extension() { check(vm_frame_drop_layer_extension(f_)); }
    // the layers through the morph: (h, w, channels) floats
    std::vector<float> render_layers(float color_fa, float geo_fa, int color_from)
    { return rendered<float>(layer_floats(), vm_render_layers, color_fa, geo_fa, color_from); }
    // ... left on the device: the kernel's milliseconds
    float render_layers_dev(float color_fa, float geo_fa, int color_from)
    { return timed(vm_render_layers_dev, color_fa, geo_fa, color_from); }

    // transition control: where the morph happens when.  Two (h, w, 2) planes of (t0, t1) in the halfway domain, for the
    // geometry and the colour (either may be nullptr: uniform (0, 1)); kept on the device until replaced or cleared
    void upload_schedule(const float *geo_t0t1, const float *color_t0t1, int pitch_floats = 0)
    {
        check(vm_frame_upload_schedule(f_, geo_t0t1, color_t0t1, pitch_floats));
    }
    void clear_schedule() { check(vm_frame_clear_schedule(f_)); }
    // render_halfway_image under the schedule at time t (vm_render_transition): the chain of render.cu:16-60 with the
    // per-texel rates in the place of geo_fa and color_fa
    std::vector<unsigned char> render_transition(float t, int ease = VM_EASE_LINEAR, int color_from = 1)
    { return rendered<unsigned char>(rgb_bytes(), vm_render_transition, t, ease, color_from); }
    float render_transition_dev(float t, int ease = VM_EASE_LINEAR, int color_from = 1)
    { return timed(vm_render_transition_dev, t, ease, color_from); }
    // the layers under the schedule: (h, w, channels) floats
    std::vector<float> render_transition_layers(float t, int ease = VM_EASE_LINEAR, int color_from = 1)
    { return rendered<float>(layer_floats(), vm_render_transition_layers, t, ease, color_from); }
    float render_transition_layers_dev(float t, int ease = VM_EASE_LINEAR, int color_from = 1)
    { return timed(vm_render_transition_layers_dev, t, ease, color_from); }
    // motion blur: render_halfway_image integrated over a shutter (vm_render_shutter) -- the mean over `samples` (1..64)
    // times between geo_open and geo_close, each clamped to [0, 1], taken in float32 before the one rounding
    std::vector<unsigned char> render_shutter(float color_fa, float geo_open, float geo_close, int samples, int color_from = 1)
    { return rendered<unsigned char>(rgb_bytes(), vm_render_shutter, color_fa, geo_open, geo_close, samples, color_from); }
    float render_shutter_dev(float color_fa, float geo_open, float geo_close, int samples, int color_from = 1)
    { return timed(vm_render_shutter_dev, color_fa, geo_open, geo_close, samples, color_from); }
    // the layers through the same shutter: (h, w, channels) floats
    std::vector<float> render_shutter_layers(float color_fa, float geo_open, float geo_close, int samples, int color_from = 1)
    { return rendered<float>(layer_floats(), vm_render_shutter_layers, color_fa, geo_open, geo_close, samples, color_from); }
    float render_shutter_layers_dev(float color_fa, float geo_open, float geo_close, int samples, int color_from = 1)
    { return timed(vm_render_shutter_layers_dev, color_fa, geo_open, geo_close, samples, color_from); }
    // motion blur under the schedule (vm_render_transition_shutter): the mean over `samples` (1..64) times between t_open
    // and t_close, the geometry schedule ramped at each of them, the colour schedule once at t_color
    std::vector<unsigned char> render_transition_shutter(float t_open, float t_close, int samples, float t_color,
                                                         int ease = VM_EASE_LINEAR, int color_from = 1)
    { return rendered<unsigned char>(rgb_bytes(), vm_render_transition_shutter, t_open, t_close, samples, t_color, ease, color_from); }
    float render_transition_shutter_dev(float t_open, float t_close, int samples, float t_color, int ease = VM_EASE_LINEAR,
                                        int color_from = 1)
    { return timed(vm_render_transition_shutter_dev, t_open, t_close, samples, t_color, ease, color_from); }
    // the layers through the same shutter and schedule: (h, w, channels) floats
    std::vector<float> render_transition_shutter_layers(float t_open, float t_close, int samples, float t_color,
                                                        int ease = VM_EASE_LINEAR, int color_from = 1)
    { return rendered<float>(layer_floats(), vm_render_transition_shutter_layers, t_open, t_close, samples, t_color, ease, color_from); }
    float render_transition_shutter_layers_dev(float t_open, float t_close, int samples, float t_color, int ease = VM_EASE_LINEAR,
                                               int color_from = 1)
    { return timed(vm_render_transition_shutter_layers_dev, t_open, t_close, samples, t_color, ease, color_from); }
    // any viewport of the morph at any size, supersampled (vm_render_viewport): every pixel of the vp.out_w x vp.out_h grid
    // the mean of vp.nx x vp.ny chains of render.cu:16-60, taken in float32 before the one rounding: (out_h, out_w, 3) bytes
    std::vector<unsigned char> render_viewport(const Viewport &vp, float color_fa, float geo_fa, int color_from = 1)
    { return rendered<unsigned char>(rgb_bytes(&vp), vm_render_viewport, &vp, color_fa, geo_fa, color_from); }
    float render_viewport_dev(const Viewport &vp, float color_fa, float geo_fa, int color_from = 1)
    { return timed(vm_render_viewport_dev, &vp, color_fa, geo_fa, color_from); }
    // the layers through the same viewport: (out_h, out_w, channels) floats
    std::vector<float> render_viewport_layers(const Viewport &vp, float color_fa, float geo_fa, int color_from = 1)
    { return rendered<float>(layer_floats(&vp), vm_render_viewport_layers, &vp, color_fa, geo_fa, color_from); }
    float render_viewport_layers_dev(const Viewport &vp, float color_fa, float geo_fa, int color_from = 1)
    { return timed(vm_render_viewport_layers_dev, &vp, color_fa, geo_fa, color_from); }
    // a viewport through a cubic filter (vm_frame_render_viewport_filtered): the taps that read the canvases take 4 x 4 texels,
    // the mean is clamped to [0, 255] before the rounding; Filter::Bilinear is render_viewport, bit for bit
    std::vector<unsigned char> render_viewport_filtered(const Viewport &vp, Filter filter, float color_fa, float geo_fa, int color_from = 1)
    { return rendered<unsigned char>(rgb_bytes(&vp), vm_frame_render_viewport_filtered, &vp, (int)filter, color_fa, geo_fa, color_from); }
    float render_viewport_filtered_dev(const Viewport &vp, Filter filter, float color_fa, float geo_fa, int color_from = 1)
    { return timed(vm_frame_render_viewport_filtered_dev, &vp, (int)filter, color_fa, geo_fa, color_from); }
    // the layers through the same viewport and filter: (out_h, out_w, channels) floats, NOT clamped (a matte may leave [0, 1])
    std::vector<float> render_viewport_filtered_layers(const Viewport &vp, Filter filter, float color_fa, float geo_fa, int color_from = 1)
    { return rendered<float>(layer_floats(&vp), vm_frame_render_viewport_filtered_layers, &vp, (int)filter, color_fa, geo_fa, color_from); }
    float render_viewport_filtered_layers_dev(const Viewport &vp, Filter filter, float color_fa, float geo_fa, int color_from = 1)
    { return timed(vm_frame_render_viewport_filtered_layers_dev, &vp, (int)filter, color_fa, geo_fa, color_from); }
    // the two plates blended band by band (vm_frame_render_multiband): render_halfway_image with color_from = 1 under the
    // multiresolution spline of `bands`, clamped to [0, 255] before the rounding: (h, w, 3) bytes
    std::vector<unsigned char> render_multiband(const Bands &bands, float color_fa, float geo_fa)
    { return rendered<unsigned char>(rgb_bytes(), vm_frame_render_multiband, &bands, color_fa, geo_fa); }
    float render_multiband_dev(const Bands &bands, float color_fa, float geo_fa)
    { return timed(vm_frame_render_multiband_dev, &bands, color_fa, geo_fa); }
    // the layers under the same bands: (h, w, channels) floats, neither clamped nor rounded
    std::vector<float> render_multiband_layers(const Bands &bands, float color_fa, float geo_fa)
    { return rendered<float>(layer_floats(), vm_frame_render_multiband_layers, &bands, color_fa, geo_fa); }
    float render_multiband_layers_dev(const Bands &bands, float color_fa, float geo_fa)
    { return timed(vm_frame_render_multiband_layers_dev, &bands, color_fa, geo_fa); }
    // ... under the schedule at time t: the colour rate k of every output pixel is the weight the bands smooth
    std::vector<unsigned char> render_multiband_transition(const Bands &bands, float t, int ease = VM_EASE_LINEAR)
    { return rendered<unsigned char>(rgb_bytes(), vm_frame_render_multiband_transition, &bands, t, ease); }
    float render_multiband_transition_dev(const Bands &bands, float t, int ease = VM_EASE_LINEAR)
    { return timed(vm_frame_render_multiband_transition_dev, &bands, t, ease); }
    std::vector<float> render_multiband_transition_layers(const Bands &bands, float t, int ease = VM_EASE_LINEAR)
    { return rendered<float>(layer_floats(), vm_frame_render_multiband_transition_layers, &bands, t, ease); }
    float render_multiband_transition_layers_dev(const Bands &bands, float t, int ease = VM_EASE_LINEAR)
    { return timed(vm_frame_render_multiband_transition_layers_dev, &bands, t, ease); }
    // diagnostic: one level of what the last multiband call left (VM_MB_G0, _G1, _MASK, _OUT): tight (h_l, w_l, C) floats,
    // C = 3 after an RGB8 call; (h_l, w_l) for the mask
    std::vector<float> multiband_level(int what, int level)
    {
        int w = w_, h = h_;
        for (int l = 0; l < level && l < VM_MULTIBAND_MAX_LEVELS; ++l) {
            w = (w + 1) / 2; h = (h + 1) / 2;
        }
        std::vector<float> out((size_t)w * h * 4);      // (at most four channels: the library knows the last call's)
        check(vm_dbg_multiband_level(f_, what, level, out.data()));
        return out;
    }
    // a viewport over a shutter (vm_render_viewport_shutter): every output pixel the mean of its vp.nx x vp.ny chains at
    // each of `samples` times between geo_open and geo_close; samples * vp.nx * vp.ny may be 256 at most
    std::vector<unsigned char> render_viewport_shutter(const Viewport &vp, float color_fa, float geo_open, float geo_close,
                                                       int samples, int color_from = 1)
    { return rendered<unsigned char>(rgb_bytes(&vp), vm_render_viewport_shutter, &vp, color_fa, geo_open, geo_close, samples, color_from); }
    float render_viewport_shutter_dev(const Viewport &vp, float color_fa, float geo_open, float geo_close, int samples,
                                      int color_from = 1)
    { return timed(vm_render_viewport_shutter_dev, &vp, color_fa, geo_open, geo_close, samples, color_from); }
    // the layers through the same viewport over the same shutter: (out_h, out_w, channels) floats
    std::vector<float> render_viewport_shutter_layers(const Viewport &vp, float color_fa, float geo_open, float geo_close,
                                                      int samples, int color_from = 1)
    { return rendered<float>(layer_floats(&vp), vm_render_viewport_shutter_layers, &vp, color_fa, geo_open, geo_close, samples, color_from); }
    float render_viewport_shutter_layers_dev(const Viewport &vp, float color_fa, float geo_open, float geo_close, int samples,
                                             int color_from = 1)
    { return timed(vm_render_viewport_shutter_layers_dev, &vp, color_fa, geo_open, geo_close, samples, color_from); }
    // a viewport over a shutter under the schedule (vm_render_viewport_transition_shutter): the geometry schedule ramped at
    // each of `samples` times between t_open and t_close, the colour schedule once at t_color
    std::vector<unsigned char> render_viewport_transition_shutter(const Viewport &vp, float t_open, float t_close, int samples,
                                                                  float t_color, int ease = VM_EASE_LINEAR, int color_from = 1)
    { return rendered<unsigned char>(rgb_bytes(&vp), vm_render_viewport_transition_shutter, &vp, t_open, t_close, samples, t_color, ease, color_from); }
    float render_viewport_transition_shutter_dev(const Viewport &vp, float t_open, float t_close, int samples, float t_color,
                                                 int ease = VM_EASE_LINEAR, int color_from = 1)
    { return timed(vm_render_viewport_transition_shutter_dev, &vp, t_open, t_close, samples, t_color, ease, color_from); }
    // the layers through the same viewport, shutter and schedule: (out_h, out_w, channels) floats
    std::vector<float> render_viewport_transition_shutter_layers(const Viewport &vp, float t_open, float t_close, int samples,
                                                                 float t_color, int ease = VM_EASE_LINEAR, int color_from = 1)
    { return rendered<float>(layer_floats(&vp), vm_render_viewport_transition_shutter_layers, &vp, t_open, t_close, samples, t_color, ease, color_from); }
    float render_viewport_transition_shutter_layers_dev(const Viewport &vp, float t_open, float t_close, int samples,
                                                        float t_color, int ease = VM_EASE_LINEAR, int color_from = 1)
    { return timed(vm_render_viewport_transition_shutter_layers_dev, &vp, t_open, t_close, samples, t_color, ease, color_from); }
    // a viewport under the schedule at the one instant t: one sample, t_open == t_close == t_color == t
    std::vector<unsigned char> render_viewport_transition(const Viewport &vp, float t, int ease = VM_EASE_LINEAR, int color_from = 1)
    {
        return render_viewport_transition_shutter(vp, t, t, 1, t, ease, color_from);
    }
    // sampling_maps under the schedule, and the rates (g, k) every output pixel ended with
    struct TransitionMaps {
        SamplingMaps maps;
        std::vector<float> rates;           // (h, w, 2): the geometric and the colour rate after the last round
    };
    TransitionMaps transition_maps(float t, int ease = VM_EASE_LINEAR)
    {
        const size_t n = (size_t)w_ * h_;
        TransitionMaps m{{std::vector<float>(2 * n), std::vector<float>(2 * n), std::vector<float>(n), std::vector<unsigned char>(n)},
                         std::vector<float>(2 * n)};
        check(vm_frame_transition_maps(f_, t, ease, m.maps.map0.data(), m.maps.map1.data(), m.maps.resid.data(), m.maps.flags.data(),
                                       m.rates.data()));
        return m;
    }

    // ---- points and motion vectors through the morph (vm_frame_carry_points, ...; image 0 is time 0, image 1 time 1)
    // n points (x, y) of the output frame at the from-time carried to nt to-times
    struct Carried {
        std::vector<float> out;                     // (nt, n, 2): the position at every to-time
        std::vector<float> halfway, pos0, pos1;     // (n, 2): in the halfway domain, in image 0, in image 1
        std::vector<float> resid;                   // n: the move of the chain's last round
        std::vector<unsigned char> flags;           // n: bit 0 / 1: pos0 / pos1 inside the image
    };
    Carried carry_points(const std::vector<float> &points_xy, float from_fa, const std::vector<float> &to_fa)
    {
        Carried c = carried(points_xy.size() / 2, to_fa.size());
        check(vm_frame_carry_points(f_, from_fa, points_xy.data(), (int)(points_xy.size() / 2), to_fa.data(), (int)to_fa.size(),
                                    c.out.data(), c.halfway.data(), c.pos0.data(), c.pos1.data(), c.resid.data(), c.flags.data(), nullptr));
        return c;
    }
    Carried carry_points_transition(const std::vector<float> &points_xy, float t_from, const std::vector<float> &t_to,
                                    int ease = VM_EASE_LINEAR)
    {
        Carried c = carried(points_xy.size() / 2, t_to.size());
        check(vm_frame_carry_points_transition(f_, t_from, ease, points_xy.data(), (int)(points_xy.size() / 2), t_to.data(),
                                               (int)t_to.size(), c.out.data(), c.halfway.data(), c.pos0.data(), c.pos1.data(),
                                               c.resid.data(), c.flags.data(), nullptr));
        return c;
    }
    // the same from every pixel centre of the output frame: out (nt, h, w, 2), resid and flags (h, w); out[k] minus the
    // pixel's own position is the motion-vector pass to time to_fa[k] (at most 16 to-times)
    struct MotionMaps {
        std::vector<float> out, resid;
        std::vector<unsigned char> flags;
    };
    MotionMaps motion_maps(float from_fa, const std::vector<float> &to_fa)
    {
        const size_t n = (size_t)w_ * h_;
        MotionMaps m{std::vector<float>(2 * n * to_fa.size()), std::vector<float>(n), std::vector<unsigned char>(n)};
        check(vm_frame_motion_maps(f_, from_fa, to_fa.data(), (int)to_fa.size(), m.out.data(), m.resid.data(), m.flags.data()));
        return m;
    }
    float motion_maps_dev(float from_fa, const std::vector<float> &to_fa)
    { return timed(vm_frame_motion_maps_dev, from_fa, to_fa.data(), (int)to_fa.size()); }
    MotionMaps transition_motion_maps(float t_from, const std::vector<float> &t_to, int ease = VM_EASE_LINEAR)
    {
        const size_t n = (size_t)w_ * h_;
        MotionMaps m{std::vector<float>(2 * n * t_to.size()), std::vector<float>(n), std::vector<unsigned char>(n)};
        check(vm_frame_transition_motion_maps(f_, t_from, ease, t_to.data(), (int)t_to.size(), m.out.data(), m.resid.data(),
                                              m.flags.data()));
        return m;
    }
    float transition_motion_maps_dev(float t_from, const std::vector<float> &t_to, int ease = VM_EASE_LINEAR)
    { return timed(vm_frame_transition_motion_maps_dev, t_from, ease, t_to.data(), (int)t_to.size()); }
    // how well each constraint is met, in pixels: (lx, ly) carried from image 0 gives pos1, compared with (rx, ry);
    // (rx, ry) carried from image 1 gives pos0, compared with (lx, ly)
    struct ConstraintGaps {
        std::vector<float> gap01, gap10;            // |pos1(l) - r|, |pos0(r) - l|
        std::vector<float> resid01, resid10;        // the resid of either carry: a gap beside a large one means little
    };
    ConstraintGaps constraint_gaps(const std::vector<vm_constraint> &cons)
    {
        if (cons.empty()) return ConstraintGaps{};
        std::vector<float> l, r;
        for (const vm_constraint &c : cons) {
            l.push_back(c.lx); l.push_back(c.ly);
            r.push_back(c.rx); r.push_back(c.ry);
        }
        const Carried a = carry_points(l, 0.0f, {1.0f}), b = carry_points(r, 1.0f, {0.0f});
        ConstraintGaps g{{}, {}, a.resid, b.resid};
        for (size_t i = 0; i < cons.size(); ++i) {
            g.gap01.push_back(std::hypot(a.pos1[2 * i] - r[2 * i], a.pos1[2 * i + 1] - r[2 * i + 1]));
            g.gap10.push_back(std::hypot(b.pos0[2 * i] - l[2 * i], b.pos0[2 * i + 1] - l[2 * i + 1]));
        }
        return g;
    }

    vm_frame *handle() const { return f_; }

private:
    static Carried carried(size_t n, size_t nt)
    {
        return Carried{std::vector<float>(2 * n * nt), std::vector<float>(2 * n), std::vector<float>(2 * n), std::vector<float>(2 * n),
                       std::vector<float>(n), std::vector<unsigned char>(n)};
    }
    // a render call that downloads, call(f_, args..., out, pitch): `count` elements, tight
    template <class T, class Call, class... Args> std::vector<T> rendered(size_t count, Call call, Args... args)
    {
        std::vector<T> out(count);
        check(call(f_, args..., out.data(), 0));
        return out;
    }
    // ... and its _dev twin, call(f_, args..., elapsed_ms): the launch's milliseconds
    template <class Call, class... Args> float timed(Call call, Args... args)
    {
        float ms = 0;
        check(call(f_, args..., &ms));
        return ms;
    }
    // the pixels of the frame, or of a viewport's output (one for a viewport the library will refuse)
    size_t pixels(const vm_viewport *vp) const
    {
        if (!vp) return (size_t)w_ * h_;
        const bool ok = vp->out_w >= 1 && vp->out_w <= 32768 && vp->out_h >= 1 && vp->out_h <= 32768;
        return ok ? (size_t)vp->out_w * vp->out_h : 1;
    }
    size_t rgb_bytes(const vm_viewport *vp = nullptr) const { return pixels(vp) * 3; }
    size_t layer_floats(const vm_viewport *vp = nullptr) const { return pixels(vp) * (channels_ ? channels_ : 1); }
    vm_frame *f_ = nullptr;
    int w_, h_, ex_;
    int channels_ = 0;
};

// CPoissonExt::run's loop body (PoissonExt.cpp:24-36) for several frames of one context at once: both sides of every
// frame are independent systems and share every launch (vm_poisson_extend_frames).  Returns the PCG iteration counts,
// [2 i] = side 1 of frames[i], [2 i + 1] = side 2.
inline std::vector<int> poisson_extend_frames(const std::vector<Frame *> &frames, float tol = 1e-5f, int max_it = 20000)
{
    std::vector<vm_frame *> h;
    for (Frame *f : frames) h.push_back(f->handle());
    std::vector<int> its(2 * h.size(), 0);
    check(vm_poisson_extend_frames(h.data(), (int)h.size(), tol, max_it, its.data(), nullptr, nullptr));
    return its;
}

} // namespace vmorph
#endif
