// examples/transition_blur.cpp -- motion blur under a transition schedule on the C++ facade: the reference's renderer
// (Algorithm/render.cu:16-60) gives one sharp instant of a uniform morph; here the morph sweeps over the frame as a wipe,
// and a shutter call integrates the moving wipe over an exposure.
//   transition_blur W H seed out_prefix
// builds a synthetic frame pair, a halfway field of up to 14 px, a matte (a float layer) and a wipe from left to right
// (the left edge starts at t = 0, the right edge 0.6 later, every texel takes 0.4) for the geometry and the colour, and
// renders the frame at t = 0.5 sharp to <out_prefix>_sharp.ppm, over a shutter 0.1 wide (0.45 .. 0.55, 16 samples, the
// colour at 0.5) to <out_prefix>_blur.ppm, and the matte through the same call to <out_prefix>_matte.pgm (binary PPM /
// PGM): the matte stays in step with the plate, because both walk the same sample times under the same rates.
// Everything is made of integer triangle waves and exact fractions, so that any host can rebuild the inputs bit for bit
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
    if (argc < 5) { fprintf(stderr, "usage: %s W H seed out_prefix\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), seed = atoi(argv[3]);
    const std::string prefix = argv[4];
    if (w < 1 || h < 1) { fprintf(stderr, "usage: %s W H seed out_prefix\n", argv[0]); return 2; }
    try {
        vmorph::Context ctx(0);
        const size_t n = (size_t)w * h;
        std::vector<unsigned char> rgb0(3 * n), rgb1(3 * n);
        std::vector<float> v(2 * n), matte0(n), matte1(n), wipe(2 * n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                for (int c = 0; c < 3; ++c) {
                    rgb0[3 * i + c] = (unsigned char)(4 * tri(3 * x + 2 * y + seed + 11 * c, 31));
                    rgb1[3 * i + c] = (unsigned char)(4 * tri(3 * (x - 4) + 2 * (y - 2) + seed + 11 * c, 31));
                }
                v[2 * i] = (float)(tri(2 * x + y + seed, 29) - 14);                 // up to 14 px, kinked
                v[2 * i + 1] = (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.5f;
                matte0[i] = (float)tri(x + y + seed, 16) * 0.0625f;                 // 0 .. 1 in sixteenths
                matte1[i] = (float)tri(x - y + seed, 16) * 0.0625f;
                wipe[2 * i] = 0.6f * ((float)x / (float)(w > 1 ? w - 1 : 1));       // t0: the start sweeps to the right
                wipe[2 * i + 1] = wipe[2 * i] + 0.4f;                               // t1
            }
        vmorph::Frame frame(ctx, w, h, 0);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        frame.upload_layers(1, matte0.data(), matte1.data());
        frame.upload_schedule(wipe.data(), wipe.data());
        const float t = 0.5f, open = 0.45f, close = 0.55f;
        const int samples = 16;
        const std::vector<unsigned char> sharp = frame.render_transition(t);
        const std::vector<unsigned char> blur = frame.render_transition_shutter(open, close, samples, t);
        const std::vector<float> matte = frame.render_transition_shutter_layers(open, close, samples, t);
        std::vector<unsigned char> grey(n);
        for (size_t i = 0; i < n; ++i) grey[i] = (unsigned char)(matte[i] * 255.0f + 0.5f);
        if (!write_pnm(prefix + "_sharp.ppm", "P6", w, h, sharp) || !write_pnm(prefix + "_blur.ppm", "P6", w, h, blur) ||
            !write_pnm(prefix + "_matte.pgm", "P5", w, h, grey))
            return 2;
        size_t moved = 0;
        for (size_t i = 0; i < 3 * n; ++i) moved += sharp[i] != blur[i];
        printf("%dx%d: a wipe at t = 0.5 sharp and over a shutter %g .. %g of %d samples; %zu of %zu bytes differ\n", w, h, open,
               close, samples, moved, 3 * n);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
