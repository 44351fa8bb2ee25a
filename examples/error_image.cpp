// examples/error_image.cpp -- the view the reference's "Error Image" menu entry promises (UI/MdiEditor.cpp:348-373,
// 1928-1933) on the C++ facade: solves a synthetic frame pair, prints the five energy totals of every level as it
// finishes, and writes the finest level's error image (heat ramp of one energy term) as a binary PPM.
//   error_image W H seed out.ppm [max_iter] [exact|fast] [what 0..4] [gain]
// The pair is a pattern of integer triangle waves, img1 = img0 moved by (2, 1) pixels, so that any host can rebuild
// it bit for bit from (W, H, seed).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vmorph/morph.hpp"

static int tri(int a, int p) { return std::abs(((a % (2 * p)) + 2 * p) % (2 * p) - p); }

static float pattern(int x, int y, int seed)
{
    return (float)(tri(3 * x + 2 * y + seed, 37) + tri(5 * y - x + 7 * seed, 53)) * (255.0f / 90.0f);
}

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: %s W H seed out.ppm [max_iter] [exact|fast] [what] [gain]\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), seed = atoi(argv[3]);
    const int what = argc > 7 ? atoi(argv[7]) : VM_ERR_SSIM;
    const float gain = argc > 8 ? (float)atof(argv[8]) : 1.0f;
    try {
        vmorph::Context ctx(0, argc > 6 && !strcmp(argv[6], "fast") ? VM_MATH_FAST : VM_MATH_EXACT);
        vmorph::Parameters params;
        params.max_iter = argc > 5 ? atoi(argv[5]) : 50;
        params.start_res = 32;
        params.max_iter_drop_factor = 1.0f;
        std::vector<float> i0((size_t)w * h), i1((size_t)w * h);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                i0[(size_t)y * w + x] = pattern(x, y, seed);
                i1[(size_t)y * w + x] = pattern(x - 2, y - 1, seed);
            }
        vmorph::Pyramid pyramid(ctx);
        pyramid.build(i0.data(), i1.data(), w, h, params.start_res);
        vmorph::MatchingThread thread(params, pyramid);
        thread.gpu_morph.keep_state = true; // the levels keep their state: the finest one is looked at below
        thread.start();
        thread.wait();
        for (auto &kv : thread.energies())
            printf("level %d %dx%d ssim %.17g tps %.17g ui %.17g temp %.17g all %.17g\n", kv.first, pyramid[kv.first].width,
                   pyramid[kv.first].height, kv.second[VM_ERR_SSIM], kv.second[VM_ERR_TPS], kv.second[VM_ERR_UI],
                   kv.second[VM_ERR_TEMP], kv.second[VM_ERR_ALL]);
        std::vector<unsigned char> rgb = pyramid[1].error_image(w, h, what, gain);
        FILE *f = fopen(argv[4], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
        fprintf(f, "P6\n%d %d\n255\n", w, h);
        fwrite(rgb.data(), 1, rgb.size(), f);
        fclose(f);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
