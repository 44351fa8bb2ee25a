// examples/multiband.cpp -- the multiband render calls on the C++ facade: the reference's renderer
// (Algorithm/render.cu:16-60; UI/RenderWidget.cpp:229-266) blends its two warped plates under one weight per pixel, so a
// dissolve at 0.5 shows both plates' detail at once and a wipe's colour seam is as wide as its ramp at every frequency; a
// multiband call blends the plates band by band, every band under the weight plane of its own scale.
//   multiband W H seed margin out_prefix
// builds zoom_filtered.cpp's synthetic frame pair and halfway field and renders, W x H pixels each:
//   <out_prefix>_dissolve_plain.ppm   render_halfway_image at color_fa = geo_fa = 0.4
//   <out_prefix>_dissolve_bands.ppm   the same instant under Bands::sharpen(L, 8): the detail of one plate, the colour of both
//                                     (at 0.5 exactly every band's weight is 0.5 whatever the table: the midpoint is where
//                                     the detail switches)
//   <out_prefix>_wipe_plain.ppm       a hard left-to-right colour wipe (no ramp) at t = 0.5 through render_transition
//   <out_prefix>_wipe_bands.ppm       the same wipe under Bands::linear(L): the seam wide in the low bands, narrow in the detail
// (binary PPM), L = Bands::for_size(W, H).  Everything is made of integer triangle waves, so that any host can rebuild the
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

static size_t differing(const std::vector<unsigned char> &a, const std::vector<unsigned char> &b)
{
    size_t n = 0;
    for (size_t i = 0; i < a.size(); i += 3) n += a[i] != b[i] || a[i + 1] != b[i + 1] || a[i + 2] != b[i + 2];
    return n;
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
                wipe[2 * i] = wipe[2 * i + 1] = (float)((double)x / (double)(w - 1));   // starts and ends at once: a hard edge
            }
        vmorph::Frame frame(ctx, w, h, margin);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        frame.upload_schedule(nullptr, wipe.data());
        const float t = 0.5f, td = 0.4f;
        const int levels = vmorph::Bands::for_size(w, h).levels;
        const std::vector<unsigned char> plain = frame.render_halfway_image(td, td, 1);
        const std::vector<unsigned char> bands = frame.render_multiband(vmorph::Bands::sharpen(levels, 8.0), td, td);
        const std::vector<unsigned char> wipe_plain = frame.render_transition(t);
        const std::vector<unsigned char> wipe_bands = frame.render_multiband_transition(vmorph::Bands::linear(levels), t);
        if (!write_ppm(prefix + "_dissolve_plain.ppm", w, h, plain) || !write_ppm(prefix + "_dissolve_bands.ppm", w, h, bands) ||
            !write_ppm(prefix + "_wipe_plain.ppm", w, h, wipe_plain) || !write_ppm(prefix + "_wipe_bands.ppm", w, h, wipe_bands))
            return 2;
        printf("%dx%d in %d levels: at t = 0.4 the sharpened dissolve differs from the plain one in %zu of %zu pixels, the multiband "
               "wipe at t = 0.5 from the hard one in %zu\n", w, h, levels, differing(plain, bands), n, differing(wipe_plain, wipe_bands));
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
