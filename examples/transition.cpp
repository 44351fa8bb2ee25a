// examples/transition.cpp -- transition control on the C++ facade: a wipe that sweeps the morph across the frame, where the
// reference's renderer (Algorithm/render.cu:16-60) moves and cross-dissolves the whole picture in lockstep.
//   transition W H seed out_prefix
// builds a synthetic frame pair and a halfway field, schedules a left-to-right wipe -- the texel of column x starts at
// t0 = 0.5 x / (W - 1) and ends half a unit of time later, geometry and colour alike -- and renders it at t = 0.25, 0.5
// and 0.75 with the smooth ease to <out_prefix>_0.ppm, _1.ppm, _2.ppm (binary PPM).  At t = 0.25 the right half is still
// image 0, at t = 0.75 the left half has arrived at image 1.  Everything is made of integer triangle waves, so that any
// host can rebuild the inputs bit for bit from (W, H, seed).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vmorph/render.hpp"

static int tri(int a, int p) { return std::abs(((a % (2 * p)) + 2 * p) % (2 * p) - p); }

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: %s W H seed out_prefix\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), seed = atoi(argv[3]);
    const std::string prefix = argv[4];
    if (w < 2 || h < 1) { fprintf(stderr, "usage: %s W H seed out_prefix (W >= 2)\n", argv[0]); return 2; }
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
                v[2 * i] = (float)(tri(2 * x + y + seed, 29) - 14) * 0.25f;         // up to 3.5 px, kinked
                v[2 * i + 1] = (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.125f;
                wipe[2 * i] = 0.5f * ((float)x / (float)(w - 1));
                wipe[2 * i + 1] = wipe[2 * i] + 0.5f;
            }
        vmorph::Frame frame(ctx, w, h, 0);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        frame.upload_schedule(wipe.data(), wipe.data());
        float worst = 0;
        for (int k = 0; k < 3; ++k) {
            const float t = 0.25f * (float)(k + 1);
            const std::vector<unsigned char> img = frame.render_transition(t, VM_EASE_SMOOTH, 1);
            const std::string name = prefix + "_" + std::to_string(k) + ".ppm";
            FILE *f = fopen(name.c_str(), "wb");
            if (!f) { fprintf(stderr, "cannot write %s\n", name.c_str()); return 2; }
            fprintf(f, "P6\n%d %d\n255\n", w, h);
            fwrite(img.data(), 1, img.size(), f);
            fclose(f);
            const vmorph::Frame::TransitionMaps m = frame.transition_maps(t, VM_EASE_SMOOTH);
            for (size_t i = 0; i < n; ++i) worst = m.maps.resid[i] > worst ? m.maps.resid[i] : worst;
        }
        printf("%dx%d: a wipe at t = 0.25, 0.5, 0.75; the last round moved %g px at most\n", w, h, worst);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
