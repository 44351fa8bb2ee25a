// examples/extend_layers.cpp -- a matte pushed through a morph whose samples leave the image, with and without the
// layers' Poisson extension (PoissonExt.cpp:49-362), on the C++ facade: what the plate gets from the extended canvases and
// its matte, until now, did not.
//   extend_layers W H ex seed out_prefix
// builds one float matte per frame and a halfway field that pushes the samples past the left and the upper edge, renders
// the matte at geo_fa = color_fa = 0.5 on the tight layers (<out_prefix>_tight.pgm: the edge texel repeats, streaks) and
// on the extended ones (<out_prefix>_ext.pgm), matte * 255 rounded, binary PGM, and writes side 1's extended matte as
// <out_prefix>_canvas.f32 (raw (H + 2 ex, W + 2 ex) float32).  The context reduces in the ordered mode, so the bytes are
// the same from run to run; everything is made of integer triangle waves, so that any host can rebuild the inputs bit for
// bit from (W, H, seed).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vmorph/render.hpp"

static int tri(int a, int p) { return std::abs(((a % (2 * p)) + 2 * p) % (2 * p) - p); }

static bool write_file(const std::string &name, const char *head, const void *data, size_t bytes)
{
    FILE *f = fopen(name.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", name.c_str()); return false; }
    fputs(head, f);
    fwrite(data, 1, bytes, f);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 6) { fprintf(stderr, "usage: %s W H ex seed out_prefix\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), ex = atoi(argv[3]), seed = atoi(argv[4]);
    const std::string prefix = argv[5];
    try {
        vmorph::Context ctx(0);
        ctx.set_reduction(VM_REDUCE_ORDERED);
        const size_t n = (size_t)w * h;
        std::vector<float> v(2 * n), matte0(n), matte1(n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                v[2 * i] = 6.0f + (float)(tri(2 * x + y + seed, 29) - 14) * 0.25f;          // 2.5 .. 9.5 px to the right
                v[2 * i + 1] = 4.0f + (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.125f; // 1.5 .. 6.5 px down
                matte0[i] = (float)tri(x + 2 * y + seed, 16) / 16.0f;                       // diagonal bars
                matte1[i] = (float)tri(3 * x - y + 2 * seed, 24) / 24.0f;
            }
        vmorph::Frame frame(ctx, w, h, ex);
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        frame.upload_layers(1, matte0.data(), matte1.data());
        char head[64];
        snprintf(head, sizeof head, "P5\n%d %d\n255\n", w, h);
        std::vector<unsigned char> grey[2];
        for (int k = 0; k < 2; ++k) {
            if (k == 1) frame.extend_layers(1e-6f);
            const std::vector<float> m = frame.render_layers(0.5f, 0.5f, 1);
            grey[k].resize(n);
            for (size_t i = 0; i < n; ++i) {
                const float g = m[i] * 255.0f + 0.5f;
                grey[k][i] = (unsigned char)(g < 0.0f ? 0.0f : g > 255.0f ? 255.0f : g);    // (the extension is not clamped)
            }
            if (!write_file(prefix + (k ? "_ext.pgm" : "_tight.pgm"), head, grey[k].data(), n)) return 2;
        }
        const std::vector<float> canvas = frame.download_layers_ext(1);
        if (!write_file(prefix + "_canvas.f32", "", canvas.data(), canvas.size() * sizeof(float))) return 2;
        const vmorph::Frame::SamplingMaps maps = frame.sampling_maps(0.5f);
        size_t outside = 0, changed = 0;
        for (size_t i = 0; i < n; ++i) {
            outside += (maps.flags[i] & 3) != 3;
            changed += grey[0][i] != grey[1][i];
        }
        printf("%dx%d, ex %d: %zu of %zu pixels sample outside an image; the extension changes %zu of them\n", w, h, ex, outside, n,
               changed);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
