// examples/carry_points.cpp -- markers, motion vectors and constraint gaps through the morph, on the C++ facade: where a
// point of one frame lies in another frame, from the fixed point the reference's renderer computes on the way to a colour
// (Algorithm/render.cu:16-60; the reference's editor never draws its lp / rp on the "Morphing result" dock).
//   carry_points W H seed out_prefix
// builds a synthetic frame pair and a halfway field (the integer triangle waves of warp_layers.cpp, so that any host can
// rebuild them bit for bit from (W, H, seed)) and
//   - carries a ring of 24 marker points of image 0 through five frames of the morph, geo_fa = 0, 0.25, 0.5, 0.75, 1:
//     <out_prefix>_ring_start.f32 (raw (24, 2) float32, x then y) and <out_prefix>_ring.f32 (raw (5, 24, 2) float32);
//   - writes the motion-vector plane of the halfway frame towards image 1 -- where every pixel of the frame at 0.5 lies at
//     time 1, minus the pixel's own position -- as <out_prefix>_mv.f32 (raw (H, W, 2) float32);
//   - prints the gaps of two constraints, one line each.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vmorph/render.hpp"

static int tri(int a, int p) { return std::abs(((a % (2 * p)) + 2 * p) % (2 * p) - p); }

static bool write_file(const std::string &name, const void *data, size_t bytes)
{
    FILE *f = fopen(name.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", name.c_str()); return false; }
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
        std::vector<float> v(2 * n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                for (int c = 0; c < 3; ++c) {
                    rgb0[3 * i + c] = (unsigned char)(4 * tri(3 * x + 2 * y + seed + 11 * c, 31));
                    rgb1[3 * i + c] = (unsigned char)(4 * tri(3 * (x - 4) + 2 * (y - 2) + seed + 11 * c, 31));
                }
                v[2 * i] = (float)(tri(2 * x + y + seed, 29) - 14) * 0.25f;
                v[2 * i + 1] = (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.125f;
            }
        vmorph::Frame frame(ctx, w, h, 0);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);

        // the markers: a ring in image 0 (time 0), drawn on five frames of the morph
        const int markers = 24;
        const float cx = 0.5f * (float)(w - 1), cy = 0.5f * (float)(h - 1), r = 0.25f * (float)(w < h ? w : h);
        std::vector<float> ring(2 * markers);
        for (int k = 0; k < markers; ++k) {
            const double a = 2.0 * 3.14159265358979323846 * k / markers;
            ring[2 * k] = cx + r * (float)std::cos(a);
            ring[2 * k + 1] = cy + r * (float)std::sin(a);
        }
        const std::vector<float> frames = {0.0f, 0.25f, 0.5f, 0.75f, 1.0f};
        const vmorph::Frame::Carried c = frame.carry_points(ring, 0.0f, frames);
        if (!write_file(prefix + "_ring_start.f32", ring.data(), ring.size() * sizeof(float))) return 2;
        if (!write_file(prefix + "_ring.f32", c.out.data(), c.out.size() * sizeof(float))) return 2;

        // the motion-vector pass of the halfway frame towards image 1
        vmorph::Frame::MotionMaps m = frame.motion_maps(0.5f, {1.0f});
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                m.out[2 * i] -= (float)x;
                m.out[2 * i + 1] -= (float)y;
            }
        if (!write_file(prefix + "_mv.f32", m.out.data(), m.out.size() * sizeof(float))) return 2;

        // two constraints: one that follows the field from the ring's first marker, one a pixel off
        const std::vector<vm_constraint> cons = {{ring[0], ring[1], c.pos1[0], c.pos1[1], 1.0f},
                                                 {ring[0], ring[1], c.pos1[0] + 1.0f, c.pos1[1], 1.0f}};
        const vmorph::Frame::ConstraintGaps g = frame.constraint_gaps(cons);
        for (size_t k = 0; k < cons.size(); ++k)
            printf("constraint %zu: 0 -> 1 misses by %.6f px (resid %.3g), 1 -> 0 by %.6f px (resid %.3g)\n", k, g.gap01[k],
                   g.resid01[k], g.gap10[k], g.resid10[k]);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
