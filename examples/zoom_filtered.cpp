// examples/zoom_filtered.cpp -- a zoom through the cubic filters on the C++ facade: the reference's renderer
// (Algorithm/render.cu:16-60) taps its colour with four texels, and its widget zooms by resampling the finished frame on
// the host (UI/RenderWidget.cpp:229-266); a filtered viewport call starts the chain wherever an output pixel lies and reads
// the plate through 4 x 4 texels.
//   zoom_filtered W H seed margin out_prefix
// builds viewport.cpp's synthetic frame pair and halfway field and a matte of its own, and renders a 4x zoom of the
// (W / 4) x (H / 4) region around a fractional centre at t = 0.5, W x H pixels each:
//   <out_prefix>_bilinear.ppm      the viewport call's own taps (Filter::Bilinear: render_viewport's bytes)
//   <out_prefix>_catmull_rom.ppm   Catmull-Rom: interpolating, sharp, overshoots (clamped to [0, 255] before the rounding)
//   <out_prefix>_mitchell.ppm      Mitchell: between sharp and smooth
//   <out_prefix>_matte.pgm         the matte through Catmull-Rom: the filtered layer call returns it unclamped, the clamp
//                                  to [0, 1] before the byte is this program's decision
// (binary PPM / PGM).  Everything is made of integer triangle waves, so that any host can rebuild the inputs bit for bit
// from (W, H, seed).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vmorph/render.hpp"

static int tri(int a, int p) { return std::abs(((a % (2 * p)) + 2 * p) % (2 * p) - p); }

static bool write_pnm(const std::string &name, const char *magic, int w, int h, const std::vector<unsigned char> &px)
{
    FILE *f = fopen(name.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", name.c_str()); return false; }
    fprintf(f, "%s\n%d %d\n255\n", magic, w, h);
    fwrite(px.data(), 1, px.size(), f);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 6) { fprintf(stderr, "usage: %s W H seed margin out_prefix\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), seed = atoi(argv[3]), margin = atoi(argv[4]);
    const std::string prefix = argv[5];
    if (w < 4 || h < 4 || margin < 0) { fprintf(stderr, "usage: %s W H seed margin out_prefix\n", argv[0]); return 2; }
    try {
        vmorph::Context ctx(0);
        const size_t n = (size_t)w * h;
        std::vector<unsigned char> rgb0(3 * n), rgb1(3 * n);
        std::vector<float> v(2 * n), matte0(n), matte1(n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                for (int c = 0; c < 3; ++c) {
                    rgb0[3 * i + c] = (unsigned char)(4 * tri(3 * x + 2 * y + seed + 11 * c, 31));
                    rgb1[3 * i + c] = (unsigned char)(4 * tri(3 * (x - 4) + 2 * (y - 2) + seed + 11 * c, 31));
                }
                v[2 * i] = (float)(tri(2 * x + y + seed, 29) - 14);                 // up to 14 px, kinked
                v[2 * i + 1] = (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.5f;
                matte0[i] = tri(x + y + seed, 8) >= 4 ? 1.0f : 0.0f;                // hard diagonal stripes: the edges ring
                matte1[i] = tri(x + y + seed - 3, 8) >= 4 ? 1.0f : 0.0f;
            }
        vmorph::Frame frame(ctx, w, h, margin);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        frame.upload_layers(1, matte0.data(), matte1.data());
        const float t = 0.5f;
        const vmorph::Viewport zoom = vmorph::Viewport::zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 4.0, w, h);
        const vmorph::Filter filters[3] = {vmorph::Filter::Bilinear, vmorph::Filter::CatmullRom, vmorph::Filter::Mitchell};
        const char *names[3] = {"_bilinear.ppm", "_catmull_rom.ppm", "_mitchell.ppm"};
        for (int k = 0; k < 3; ++k)
            if (!write_pnm(prefix + names[k], "P6", w, h, frame.render_viewport_filtered(zoom, filters[k], t, t, 1)))
                return 2;
        const std::vector<float> matte = frame.render_viewport_filtered_layers(zoom, vmorph::Filter::CatmullRom, t, t, 1);
        std::vector<unsigned char> grey(n);
        size_t outside = 0;
        for (size_t i = 0; i < n; ++i) {
            const float m = matte[i];
            outside += m < 0.0f || m > 1.0f;
            grey[i] = (unsigned char)((m < 0.0f ? 0.0f : m > 1.0f ? 1.0f : m) * 255.0f + 0.5f);
        }
        if (!write_pnm(prefix + "_matte.pgm", "P5", w, h, grey))
            return 2;
        printf("%dx%d at t = 0.5: a 4x zoom from (%g, %g) in bilinear, Catmull-Rom and Mitchell; the matte through Catmull-Rom "
               "leaves [0, 1] in %zu of %zu pixels\n", w, h, zoom.x0, zoom.y0, outside, n);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
