// vmorph/track.hpp -- C++ host mirror of the key-point edits of stage 2: MdiEditor::AddPoint /
// MovePoint (UI/MdiEditor.cpp:1230-1393), the stage-2 branch of ConnectPoint (:1395-1475) and
// NextStage's points section (:1714-1791), on vmorph::Parameters over a PointTracker (vm_track:
// resample1/2, f1/f2, b1/b2 on the device).  The same operations as videomorphing_amd/morph.py's
// PointTracker, Parameters.add_point / move_point / connect_point and stage_two_parameters.
#ifndef VMORPH_TRACK_HPP
#define VMORPH_TRACK_HPP

#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

#include "video.hpp"

namespace vmorph {

class PointTracker {
public:
    // two RGB8 videos (h*w*3 bytes per frame, depth frames each); flows == nullptr: computed on the
    // device (vm_track_compute_flows), else flows[k][t] = f0, f1, b0, b1 of frame t (h*w*2 floats)
    PointTracker(Context &ctx, const std::vector<const unsigned char *> &video0, const std::vector<const unsigned char *> &video1,
                 int w, int h, const std::vector<const float *> *flows = nullptr, const vm_flow_params *flow_params = nullptr)
        : depth((int)video0.size())
    {
        if (video1.size() != video0.size()) throw std::invalid_argument("vmorph::PointTracker: videos of different length");
        check(vm_track_create(ctx.handle(), w, h, depth, &h_));
        try {
            for (int t = 0; t < depth; ++t) {
                check(vm_track_upload_frame(h_, 0, t, video0[t], 0));
                check(vm_track_upload_frame(h_, 1, t, video1[t], 0));
            }
            if (!flows) {
                check(vm_track_compute_flows(h_, flow_params));
            } else {
                for (int side = 0; side < 2; ++side)
                    for (int t = 0; t < depth; ++t)
                        check(vm_track_upload_flows(h_, side, t, flows[side][t], flows[2 + side][t], 0));
            }
        } catch (...) {
            vm_track_destroy(h_);
            throw;
        }
    }
    ~PointTracker() { vm_track_destroy(h_); }
    PointTracker(const PointTracker &) = delete;
    PointTracker &operator=(const PointTracker &) = delete;
    vm_track *handle() const { return h_; }

    // vm_track_propagate: row i of the result (depth points) holds segment i's covered frames, zeros elsewhere
    std::vector<vm_track_point> propagate(const std::vector<vm_track_segment> &segs)
    {
        std::vector<vm_track_point> out(segs.size() * (size_t)depth, vm_track_point{0, 0, 0.f});
        check(vm_track_propagate(h_, segs.data(), (int)segs.size(), out.data()));
        return out;
    }

    const int depth;

private:
    vm_track *h_ = nullptr;
};

namespace track_detail {

// a chain from key k (int4 p: x, y, frame) in direction dir, or the blend from the moved key m towards o
inline vm_track_segment chain(int side, const int4 &k, int dir) { return {side, k.x, k.y, k.z, 0, 0, -1, dir}; }
inline vm_track_segment blend(int side, const int4 &m, const int4 &o) { return {side, m.x, m.y, m.z, o.x, o.y, o.z, 0}; }

// writes segment s's covered frames of row `row` into the track
inline void apply(std::vector<Conp> &track, const vm_track_segment &s, const vm_track_point *row, int d)
{
    int a, b;
    if (s.ofr < 0) {
        a = s.dir > 0 ? s.frame + 1 : 0;
        b = s.dir > 0 ? d : s.frame;
    } else {
        a = std::min(s.frame, s.ofr) + 1;
        b = std::max(s.frame, s.ofr);
    }
    for (int t = a; t < b; ++t) track[t] = Conp{{row[t].x, row[t].y, t, 0}, row[t].weight};
}

inline std::vector<std::vector<Conp>> &points(Parameters &P, int side) { return side == 0 ? P.lp : P.rp; }

} // namespace track_detail

// MdiEditor::AddPoint (UI/MdiEditor.cpp:1230-1276): a new track of `side` (0 = lp, 1 = rp) from the key (x, y)
// at `frame`, walked through every other frame; returns the track's index
inline int add_point(Parameters &P, int side, int x, int y, int frame, PointTracker &tracker)
{
    using namespace track_detail;
    const int d = tracker.depth;
    const int4 key{x, y, frame, 1};
    const std::vector<vm_track_segment> segs{chain(side, key, -1), chain(side, key, 1)};
    const std::vector<vm_track_point> out = tracker.propagate(segs);
    std::vector<Conp> track(d, Conp{{0, 0, 0, 0}, 0.f});
    track.at(frame) = Conp{key, 1.0f};
    for (size_t i = 0; i < segs.size(); ++i) apply(track, segs[i], out.data() + i * d, d);
    points(P, side).push_back(track);
    return (int)points(P, side).size() - 1;
}

// MdiEditor::MovePoint (UI/MdiEditor.cpp:1279-1393): the key of `track` at `frame` becomes (x, y); the frames
// up to the neighbouring keys (or the ends) are propagated again, blended with the neighbours' chains
inline void move_point(Parameters &P, int side, int track, int frame, int x, int y, PointTracker &tracker)
{
    using namespace track_detail;
    std::vector<Conp> &pts = points(P, side).at(track);
    const int d = (int)pts.size();
    const int4 m{x, y, frame, 1};
    pts.at(frame) = Conp{m, 1.0f};
    int beg = -1, end = -1;
    for (int j = frame - 1; j >= 0 && beg < 0; --j)
        if (pts[j].p.w) beg = j;
    for (int j = frame + 1; j < d && end < 0; ++j)
        if (pts[j].p.w) end = j;
    const std::vector<vm_track_segment> segs{beg < 0 ? chain(side, m, -1) : blend(side, m, pts[beg].p),
                                             end < 0 ? chain(side, m, 1) : blend(side, m, pts[end].p)};
    const std::vector<vm_track_point> out = tracker.propagate(segs);
    for (size_t i = 0; i < segs.size(); ++i) apply(pts, segs[i], out.data() + i * tracker.depth, d);
}

// the stage-2 branch of MdiEditor::ConnectPoint (UI/MdiEditor.cpp:1395-1475, thread_flag >= 2): a per-frame
// list (l_track, t) - (r_track, t) is added when neither track is connected, removed when exactly this pair is;
// nothing happens when only one of them is connected elsewhere
inline void connect_point(Parameters &P, int l_track, int r_track)
{
    for (size_t k = 0; k < P.cnt.size(); ++k)
        for (const Connect &c : P.cnt[k])
            if (c.li.x == l_track || c.ri.x == r_track) {
                if (c.li.x == l_track && c.ri.x == r_track) P.cnt.erase(P.cnt.begin() + k);
                return;
            }
    std::vector<Connect> row;
    for (int t = 0; t < (int)P.lp.at(l_track).size(); ++t) row.push_back(Connect{{l_track, t}, {r_track, t}});
    P.cnt.push_back(row);
}

// NextStage's points section (UI/MdiEditor.cpp:1714-1791) in the segment form, ONE vm_track_propagate call for
// both sides: connection j of stage-1 list i becomes a key at ((x, y), (lz + rz) / 2) on track i of either side,
// list i becomes the d connects (i, t) - (i, t).  An empty stage-1 list is an error.
inline Parameters stage_two_parameters(const Parameters &P_sync, PointTracker &tracker)
{
    using namespace track_detail;
    const int d = tracker.depth;
    const size_t n = P_sync.cnt.size();
    std::vector<std::map<int, std::pair<int4, int>>> keys[2]; // per side, per list: frame -> (key, last edit)
    for (int side = 0; side < 2; ++side) keys[side].resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (P_sync.cnt[i].empty()) throw std::invalid_argument("vmorph::stage_two_parameters: stage-1 connection list is empty");
        for (size_t j = 0; j < P_sync.cnt[i].size(); ++j) {
            const Connect &c = P_sync.cnt[i][j];
            const int4 &l = P_sync.lp.at(c.li.x).at(c.li.y).p, &r = P_sync.rp.at(c.ri.x).at(c.ri.y).p;
            const int z = (int)((l.z + r.z) / 2 + 0.5);
            keys[0][i][z] = {int4{l.x, l.y, z, 1}, (int)j};
            keys[1][i][z] = {int4{r.x, r.y, z, 1}, (int)j};
        }
    }
    std::vector<vm_track_segment> segs;
    std::vector<std::pair<int, size_t>> owner; // (side, list) of each segment
    for (int side = 0; side < 2; ++side)
        for (size_t i = 0; i < n; ++i) {
            const auto &kk = keys[side][i];
            segs.push_back(chain(side, kk.begin()->second.first, -1));
            segs.push_back(chain(side, kk.rbegin()->second.first, 1));
            for (auto a = kk.begin(), b = std::next(a); b != kk.end(); ++a, ++b)
                segs.push_back(a->second.second > b->second.second ? blend(side, a->second.first, b->second.first)
                                                                   : blend(side, b->second.first, a->second.first));
            while (owner.size() < segs.size()) owner.push_back({side, i});
        }
    const std::vector<vm_track_point> out = tracker.propagate(segs);
    Parameters P = P_sync;
    P.lp.assign(n, std::vector<Conp>(d, Conp{{0, 0, 0, 0}, 0.f}));
    P.rp = P.lp;
    P.cnt.clear();
    for (int side = 0; side < 2; ++side)
        for (size_t i = 0; i < n; ++i)
            for (const auto &k : keys[side][i]) points(P, side)[i].at(k.first) = Conp{k.second.first, 1.0f};
    for (size_t s = 0; s < segs.size(); ++s)
        apply(points(P, owner[s].first)[owner[s].second], segs[s], out.data() + s * d, d);
    for (size_t i = 0; i < n; ++i) {
        std::vector<Connect> row;
        for (int t = 0; t < d; ++t) row.push_back(Connect{{(int)i, t}, {(int)i, t}});
        P.cnt.push_back(row);
    }
    return P;
}

// the flow half of Pyramid::build from the tracker's flows, device to device (vm_video_build_flows_track)
inline void build_flows_track(VideoPyramid &video, const PointTracker &tracker)
{
    check(vm_video_build_flows_track(video.handle(), tracker.handle()));
}

} // namespace vmorph
#endif
