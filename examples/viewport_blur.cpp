// examples/viewport_blur.cpp -- viewports over a shutter on the C++ facade: the reference's renderer
// (Algorithm/render.cu:16-60) gives one sharp instant of the w x h grid, and its widget zooms by resampling that frame on
// the host (UI/RenderWidget.cpp:229-266); here a viewer zooms into a motion-blurred frame and a proxy of a wipe is
// delivered at half size, each in one call that filters the morph and not the finished picture.
//   viewport_blur W H seed out_prefix
// builds transition_blur.cpp's synthetic frame pair, halfway field of up to 14 px and wipe from left to right, and writes
//   <out_prefix>_zoom.ppm    a 2.5x zoom around a fractional centre, (W / 2) x (H / 2) pixels, of the uniform morph over a
//                            shutter 0.4 .. 0.6 of 16 samples, the colour at 0.5
//   <out_prefix>_proxy.ppm   the whole frame at half size, 2 x 2 samples per pixel, under the wipe over a shutter
//                            0.45 .. 0.55 of 16 samples, the colour at 0.5
//   <out_prefix>_still.ppm   the same proxy of the wipe at the one instant t = 0.5
// (binary PPM).  Everything is made of integer triangle waves and exact fractions, so that any host can rebuild the
// inputs bit for bit from (W, H, seed).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vmorph/render.hpp"

static int tri(int a, int p) { return std::abs(((a % (2 * p)) + 2 * p) % (2 * p) - p); }

static bool write_ppm(const std::string &name, int w, int h, const std::vector<unsigned char> &px)
{
    FILE *f = fopen(name.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", name.c_str()); return false; }
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    fwrite(px.data(), 1, px.size(), f);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: %s W H seed out_prefix\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), seed = atoi(argv[3]);
    const std::string prefix = argv[4];
    if (w < 2 || h < 2) { fprintf(stderr, "usage: %s W H seed out_prefix\n", argv[0]); return 2; }
    try {
        vmorph::Context ctx(0);
        const size_t n = (size_t)w * h;
        std::vector<unsigned char> rgb0(3 * n), rgb1(3 * n);
        std::vector<float> v(2 * n), wipe(2 * n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                for (int c = 0; c < 3; ++c) {
                    rgb0[3 * i + c] = (unsigned char)(4 * tri(3 * x + 2 * y + seed + 11 * c, 31));
                    rgb1[3 * i + c] = (unsigned char)(4 * tri(3 * (x - 4) + 2 * (y - 2) + seed + 11 * c, 31));
                }
                v[2 * i] = (float)(tri(2 * x + y + seed, 29) - 14);                 // up to 14 px, kinked
                v[2 * i + 1] = (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.5f;
                wipe[2 * i] = 0.6f * ((float)x / (float)(w - 1));                   // t0: the start sweeps to the right
                wipe[2 * i + 1] = wipe[2 * i] + 0.4f;                               // t1
            }
        vmorph::Frame frame(ctx, w, h, 0);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        frame.upload_schedule(wipe.data(), wipe.data());
        const float t = 0.5f;
        const int samples = 16;
        const vmorph::Viewport zoom = vmorph::Viewport::zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 2.5, w / 2, h / 2);
        const vmorph::Viewport proxy = vmorph::Viewport::fit(w, h, w / 2, h / 2).supersampled(2);
        if (!write_ppm(prefix + "_zoom.ppm", zoom.out_w, zoom.out_h, frame.render_viewport_shutter(zoom, t, 0.4f, 0.6f, samples)) ||
            !write_ppm(prefix + "_proxy.ppm", proxy.out_w, proxy.out_h,
                       frame.render_viewport_transition_shutter(proxy, 0.45f, 0.55f, samples, t)) ||
            !write_ppm(prefix + "_still.ppm", proxy.out_w, proxy.out_h, frame.render_viewport_transition(proxy, t)))
            return 2;
        printf("%dx%d: a 2.5x zoom of %dx%d from (%g, %g) over a shutter of %d samples, a %dx%d proxy of 2x2 samples of a wipe over one "
               "and at t = 0.5\n", w, h, zoom.out_w, zoom.out_h, zoom.x0, zoom.y0, samples, proxy.out_w, proxy.out_h);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
