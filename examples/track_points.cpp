// examples/track_points.cpp -- the key-point edits of stage 2 through the C++ facade: the flows of both
// videos on the device (PointTracker), NextStage's conversion of stage-1 connections into tracks, then one
// AddPoint per side, a MovePoint and a ConnectPoint.
//   track_points W H D frames.u8 cons.i32 NCONS out.i32
// frames.u8: D x 2 RGB8 frames (video 0 frame t, video 1 frame t, ...); cons.i32: NCONS x (list lx ly lz rx ry rz),
// stage-1 connections (each its own one-point track per side) grouped into lists 0, 1, ... in order.
// out.i32: the number of lp tracks, rp tracks and cnt lists; every lp then rp track as D x (x y z w weight-bits);
// every cnt list as its length followed by (li.x li.y ri.x ri.y) per connection.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vmorph/track.hpp"

template <class T> static std::vector<T> read_all(const char *path, size_t n)
{
    std::vector<T> v(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 8) { fprintf(stderr, "usage: %s W H D frames.u8 cons.i32 NCONS out.i32\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), d = atoi(argv[3]), ncons = atoi(argv[6]);
    try {
        const size_t frame = (size_t)w * h * 3;
        std::vector<unsigned char> frames = read_all<unsigned char>(argv[4], frame * 2 * d);
        std::vector<int> cons = read_all<int>(argv[5], (size_t)ncons * 7);
        vmorph::Context ctx(0);
        std::vector<const unsigned char *> v0, v1;
        for (int t = 0; t < d; ++t) {
            v0.push_back(frames.data() + frame * (2 * t));
            v1.push_back(frames.data() + frame * (2 * t + 1));
        }
        vmorph::PointTracker tracker(ctx, v0, v1, w, h);
        vmorph::Parameters sync;
        for (int k = 0; k < ncons; ++k) {
            const int *q = &cons[7 * k];
            sync.lp.push_back({vmorph::Conp{{q[1], q[2], q[3], 1}, 1.0f}});
            sync.rp.push_back({vmorph::Conp{{q[4], q[5], q[6], 1}, 1.0f}});
            if (q[0] >= (int)sync.cnt.size()) sync.cnt.resize(q[0] + 1);
            sync.cnt[q[0]].push_back(vmorph::Connect{{k, 0}, {k, 0}});
        }
        vmorph::Parameters P = vmorph::stage_two_parameters(sync, tracker);
        const int a = vmorph::add_point(P, 0, w / 3, h / 2, d - 1, tracker);
        const int b = vmorph::add_point(P, 1, w / 2, h / 2, d / 2, tracker);
        vmorph::move_point(P, 0, a, 0, w / 2, h / 3, tracker);
        vmorph::connect_point(P, a, b);
        std::vector<int> out{(int)P.lp.size(), (int)P.rp.size(), (int)P.cnt.size()};
        for (const auto *side : {&P.lp, &P.rp})
            for (const auto &track : *side)
                for (const vmorph::Conp &c : track) {
                    int bits;
                    std::memcpy(&bits, &c.weight, 4);
                    out.insert(out.end(), {c.p.x, c.p.y, c.p.z, c.p.w, bits});
                }
        for (const auto &row : P.cnt) {
            out.push_back((int)row.size());
            for (const vmorph::Connect &c : row) out.insert(out.end(), {c.li.x, c.li.y, c.ri.x, c.ri.y});
        }
        FILE *f = fopen(argv[7], "wb");
        if (!f || fwrite(out.data(), sizeof(int), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
        fclose(f);
        printf("%zu + %zu tracks of %d frames, %zu connection lists\n", P.lp.size(), P.rp.size(), d, P.cnt.size());
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
