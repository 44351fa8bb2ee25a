// examples/warp_layers.cpp -- a matte carried through the morph, and the dense correspondence itself, on the C++ facade:
// what the reference's renderer computes on the way to a colour and throws away (Algorithm/render.cu:16-60).
//   warp_layers W H seed out_prefix
// builds a synthetic frame pair, a halfway field and one float matte per frame, carries the mattes through the morph at
// geo_fa = color_fa = 0, 0.5 and 1 and writes them as <out_prefix>_0.pgm, _1.pgm, _2.pgm (binary PGM, matte * 255
// rounded), and writes the forward map image 0 -> image 1 -- the image-1 sampling positions at geo_fa = 0 -- as
// <out_prefix>_forward.f32 (raw (H, W, 2) float32, x then y, in image pixels).  Everything is made of integer
// triangle waves, so that any host can rebuild the inputs bit for bit from (W, H, seed).
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
    if (argc < 5) { fprintf(stderr, "usage: %s W H seed out_prefix\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), seed = atoi(argv[3]);
    const std::string prefix = argv[4];
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
                v[2 * i] = (float)(tri(2 * x + y + seed, 29) - 14) * 0.25f;         // up to 3.5 px, kinked
                v[2 * i + 1] = (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.125f;
                matte0[i] = (float)tri(x + seed, 16) / 16.0f;                       // vertical bars
                matte1[i] = (float)tri(y + 2 * seed, 16) / 16.0f;                   // horizontal bars
            }
        vmorph::Frame frame(ctx, w, h, 0);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        frame.upload_layers(1, matte0.data(), matte1.data());
        char head[64];
        snprintf(head, sizeof head, "P5\n%d %d\n255\n", w, h);
        for (int k = 0; k < 3; ++k) {
            const float fa = 0.5f * (float)k;
            const std::vector<float> m = frame.render_layers(fa, fa, 1);
            std::vector<unsigned char> grey(n);
            for (size_t i = 0; i < n; ++i) grey[i] = (unsigned char)(m[i] * 255.0f + 0.5f);
            if (!write_file(prefix + "_" + std::to_string(k) + ".pgm", head, grey.data(), n)) return 2;
        }
        const vmorph::Frame::SamplingMaps maps = frame.sampling_maps(0.0f);
        if (!write_file(prefix + "_forward.f32", "", maps.map1.data(), maps.map1.size() * sizeof(float))) return 2;
        size_t outside = 0;
        float worst = 0;
        for (size_t i = 0; i < n; ++i) {
            outside += (maps.flags[i] & 2) == 0;
            worst = maps.resid[i] > worst ? maps.resid[i] : worst;
        }
        printf("%dx%d: %zu of %zu pixels sample image 1 outside the frame; the last round moved %g px at most\n", w, h, outside, n, worst);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
