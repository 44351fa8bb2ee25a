// vm_mgb_plan.h -- the host rules of the compositor's linear solver (vm_mgb.h), as pure code: the constants, the
// hierarchy of a grid (sizes, tail, sweeps per level), the layout of a system's workspace and of its ordered-mode
// storage, the host's folds of the residual norm, and the rule by which a system of a batch stops.  No HIP here: plain
// g++ compiles this header (tests/test_mgb_plan.py); the driver that acts on it is vm_poisson_api.cpp.
#ifndef VM_MGB_PLAN_H
#define VM_MGB_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>

#define VM_MGB_MAXLEV 14
#define VM_MGB_SLOTS 8          // dot-product accumulators are spread over 8 lines: same-address double atomics serialise in the L2
#define VM_MGB_MAXSYS 64

// a vector entry in memory: three colour channels, 12 bytes (dwordx3 loads / stores: a quarter less traffic than float4)
struct VmV3 {
    float x, y, z;
};

struct VmMgbScalars {
    double bb[VM_MGB_SLOTS][16];        // [slot][channel], one 128-byte line per slot
    double rr[2][VM_MGB_SLOTS][16];     // [iteration parity] ...
    double rz[2][VM_MGB_SLOTS][16];
    double pq[2][VM_MGB_SLOTS][16];
};

// ---------------------------------------------------------------------------
// ORDERED reduction (vm_set_reduction(ctx, VM_REDUCE_ORDERED); the default, VM_REDUCE_ATOMIC, is the slots above).
// Every dot product of the PCG becomes a fold in ONE fixed order that is a function of the system alone:
//   * a producing workgroup is entry i of the system's OWN list of the launch -- i < n, n = ceil(nblocks / MGB_G) in the
//     streaming kernels (init, dirspmv, update, dot_rz), n = ntiles of level 0 in the tile kernels (the fused update in
//     the restriction, the prolongation) -- and leaves the three channel sums of its cells (the same shuffle tree and
//     wave order as the default) in part[acc][i].  Workgroups the launch holds beyond n (the grid is the batch's
//     maximum) publish nothing and take no ticket;
//   * workgroups i with the same i / VM_MGB_ORD_GROUP share an arrival ticket; the one that arrives LAST adds the
//     group's partials in ascending i from zero into gpart[acc][i / VM_MGB_ORD_GROUP] and resets the ticket.  Nobody
//     waits for anybody;
//   * the consumers -- the NEXT launch, where the default sums its slots, and the host's stop test -- fold the
//     ng = ceil(n / VM_MGB_ORD_GROUP) group partials: on the device lane j of 32 adds entries j, j + 32, ... in ascending
//     order from zero and the 32 lanes are joined by a butterfly (xor 16, 8, 4, 2, 1); the host adds entries 0 .. ng - 1
//     in ascending order (bb and rr, which only the host reads).
// gridDim, the batch-mates, the system's index, the stream and the context do not enter.  The fused and the separate
// update partition level 0 by tiles and by blocks: their ordered bits may differ (VM_MGB_FUSE_MIN_SYS is a dev switch).
#define VM_MGB_ORD_GROUP 32
#define VM_MGB_ORD_TSTRIDE 32   // words between tickets: one 128-byte line each
enum { VM_MGB_ACC_BB = 0, VM_MGB_ACC_RR = 1, VM_MGB_ACC_RZ = 3, VM_MGB_ACC_PQ = 5, VM_MGB_NACC = 7 };   // + the iteration's parity
struct VmMgbOrd {               // one system's storage (device), constant during a solve
    int cap, gcap;              // producing workgroups / groups there is room for
    double *part;               // [VM_MGB_NACC][cap][4]: a workgroup's channel sums (written through, read by its group's last arriver)
    double *gpart;              // [VM_MGB_NACC][gcap][4]: the groups' sums
    unsigned *ticket;           // [VM_MGB_NACC][gcap] x VM_MGB_ORD_TSTRIDE words, zero between launches
    int *ng;                    // [VM_MGB_NACC]: groups of the launch that last produced the accumulator
};

#define VM_MGB_COARSEST 64      // the hierarchy ends at a grid of at most this many cells ...
// Red-black sweeps each way per level, from level 0 on (comma list, the last entry repeats; mg_nu below).
// Measured on the 2304 x 1464 canvas, tol 1e-5 / 1e-6 (tools/exp/nu_sweep.sh, nu_ab.sh on one box; tools/exp/mg_prototype.py
// is the CPU model that predicted the iteration counts), ms per frame in 4-frame batches in the bench line's setting:
//   1 everywhere      11 / 13 iterations   2.20 / 2.52
//   1, 1, 2           9 / 10               2.00 / 2.17   <- the extra sweeps go where the cycle is launch-bound, not byte-bound
//   2 everywhere      7-8 / 8              as slow as 1 everywhere: level 0's wider window costs what the iterations save
// The quadratic path's whole-grid system (1920 x 1080, tol 1e-4, a solved field) stays at 1 everywhere: 1.72 ms (8 iterations)
// against 2.02 (8) with 1, 1, 2 and 1.89 (6) with 2 everywhere.
#ifndef VM_MGB_NU_POISSON
#define VM_MGB_NU_POISSON 1, 1, 2
#define VM_MGB_NU_QPATH 1
#endif
#define VM_MGB_COARSE_SWEEPS 2  // ... which gets this many symmetric Gauss-Seidel sweeps each way (R B R B, B R B R) from zero
// the tail of the cycle -- every level from `tail` on -- runs in ONE workgroup with the iterates in LDS: the levels'
// cell counts must fit these pools: all of them (a float4 iterate + a float2 of edge weights per cell) / all but the first
// (a float4 right-hand side): 120 + 32 KB of the CU's 160 KB of LDS
#ifndef VM_MGB_TAIL_X
#define VM_MGB_TAIL_X 5120
#define VM_MGB_TAIL_B 2048
#endif
// ... and no level of the tail may hold more than this many PAIRS of cells, ceil(w / 2) h (the tail's threads are dealt
// pairs, three each)
#ifndef VM_MGB_TAIL_PAIRS
#define VM_MGB_TAIL_PAIRS 3072
#endif

// ---------------------------------------------------------------------------
// The hierarchy of a w x h grid

typedef std::vector<std::pair<int, int>> MgSizes;   // (w, h) per level

// grid sizes: halve (rounding up) down to a grid of at most VM_MGB_COARSEST cells
inline MgSizes mg_sizes(int w, int h)
{
    MgSizes v{{w, h}};
    while ((size_t)v.back().first * v.back().second > VM_MGB_COARSEST && (int)v.size() < VM_MGB_MAXLEV)
        v.push_back({(v.back().first + 1) / 2, (v.back().second + 1) / 2});
    return v;
}

// the first level of the cycle's one-workgroup tail: from there on all iterates fit VM_MGB_TAIL_X cells of LDS and all
// right-hand sides but the first VM_MGB_TAIL_B
inline int mg_tail_level(const MgSizes &sz)
{
    size_t below = 0;       // cells of the levels after l
    int l = (int)sz.size() - 1;
    while (l > 0) {
        const size_t here = (size_t)sz[l].first * sz[l].second, up = (size_t)sz[l - 1].first * sz[l - 1].second;
        if (below + here + up > VM_MGB_TAIL_X || below + here > VM_MGB_TAIL_B ||
            (size_t)((sz[l - 1].first + 1) / 2) * sz[l - 1].second > VM_MGB_TAIL_PAIRS)
            break;
        below += here;
        --l;
    }
    return l;
}

// VM_MGB_NU's syntax: every digit 1 .. 9 is an entry
inline std::vector<int> mg_parse_nu(const char *text)
{
    std::vector<int> t;
    for (const char *q = text; *q; ++q)
        if (*q >= '1' && *q <= '9') t.push_back(*q - '0');
    return t;
}

// The environment's development switches over the solver's rules.
struct MgbSwitches {
    std::vector<int> nu;    // VM_MGB_NU = "a,b,c": sweeps per level for both kinds of system (mg_nu); empty: the measured tables
    int fuse_min = 1;       // VM_MGB_FUSE_MIN_SYS: the smallest batch that fuses (0: never)

    // the process' switches, read from the environment once
    static const MgbSwitches &from_environment()
    {
        static const MgbSwitches sw = [] {
            MgbSwitches s;
            if (const char *e = getenv("VM_MGB_NU")) s.nu = mg_parse_nu(e);
            if (const char *e = getenv("VM_MGB_FUSE_MIN_SYS")) s.fuse_min = atoi(e);
            return s;
        }();
        return sw;
    }
};

// red-black sweeps each way on level l of the cycle (VmMgbLevel::nu), by kind of system: VM_MGB_NU_POISSON / _QPATH
// (above: measured choices).  VM_MGB_NU = "a,b,c" overrides both for experiments: sweeps per level from level 0 on, the
// last entry repeats; 1 or 2 on the levels the tile kernels sweep (larger values are cut to 2 there), 1 .. 9 inside the
// one-workgroup tail
inline const std::vector<int> &mg_nu_table(const MgbSwitches &sw, bool qpath)
{
    static const std::vector<int> poisson{VM_MGB_NU_POISSON}, path{VM_MGB_NU_QPATH};
    return !sw.nu.empty() ? sw.nu : qpath ? path : poisson;
}

inline int mg_nu(const std::vector<int> &table, int l, bool in_tail)
{
    const int nu = table[std::min((size_t)l, table.size() - 1)];
    return in_tail ? nu : std::min(nu, 2);
}

// The PCG update can ride in the level-0 restriction wherever that kernel exists in its one-sweep form: level 0 swept by
// the tile kernels (not inside the tail) with one sweep each way (nu0) -- and it does wherever the hierarchy allows it.
// Measured on the 2304 x 1464 canvas (tools/exp/fuse_ab.sh, ms per frame at 1e-5, fused against the separate k_mgb_update):
// 8 systems per batch 1.61 / 1.70, 4 systems 1.95 / 1.99, 2 systems 2.49 / 2.51, one system 1.78 / 1.81 per side (with the
// fused kernel's loads issued cell by cell it lost on one and two systems, 2.56 / 2.49: vm_mgb.hip).  Same arithmetic
// either way.  fuse_min: MgbSwitches (dev switch)
inline bool mgb_fused(int tail, int nu0, int fuse_min, int nsys)
{
    return tail > 0 && nu0 == 1 && fuse_min > 0 && nsys >= fuse_min;
}

// ---------------------------------------------------------------------------
// One system's device workspace: the offset of every array from the workspace's base, in the order they lie, each
// aligned to 256 bytes.  The driver carves pointers from it (vm_poisson_api.cpp: mgb_carve); `bytes` is what it reserves.

inline size_t mgb_align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct MgbLevelLayout {
    int w, h;
    int gx, gy;                 // blocks of 64 x 4 cells covering the grid
    size_t info;                // level 0: one byte of operator per cell
    size_t we, ws, dg, k;       // levels >= 1: a float per cell each
    size_t b, xr, flags, blocks, tiles;
    size_t x;
};

struct MgbLayout {
    int nlev, tail;             // tail: first level of the cycle's one-workgroup tail
    size_t type, sc, counts;    // counts: nblocks per level, then ntiles per level
    size_t X, P[2], Q, r1;      // r1: second buffer of the PCG residual (mgb_fused)
    MgbLevelLayout lv[VM_MGB_MAXLEV];
    size_t xcoarse, xcoarse_bytes;  // the x arrays of levels >= 1, contiguous (cleared per extension)
    size_t xbest;               // with_best: room for one more iterate, past everything else (the quadratic path keeps the best one seen: MgbStop)
    size_t bytes;

    MgbLayout(int w, int h, bool with_best)
    {
        const MgSizes sz = mg_sizes(w, h);
        const size_t N0 = (size_t)w * h;
        size_t off = 0;
        auto take = [&off](size_t n) { const size_t o = off; off += mgb_align256(n); return o; };
        nlev = (int)sz.size();
        tail = mg_tail_level(sz);
        type = take(N0); sc = take(sizeof(VmMgbScalars)); counts = take(2 * VM_MGB_MAXLEV * sizeof(int));
        X = take(N0 * 12); P[0] = take(N0 * 12); P[1] = take(N0 * 12); Q = take(N0 * 12); r1 = take(N0 * 12);
        for (int l = 0; l < nlev; ++l) {
            MgbLevelLayout &L = lv[l];
            L.w = sz[l].first; L.h = sz[l].second;
            L.gx = (L.w + 63) / 64; L.gy = (L.h + 3) / 4;
            const size_t N = (size_t)L.w * L.h, nb = (size_t)L.gx * L.gy;
            L.info = L.we = L.ws = L.dg = L.k = 0;
            if (l == 0) {
                L.info = take(N);
            } else {
                L.we = take(N * 4); L.ws = take(N * 4); L.dg = take(N * 4); L.k = take(N * 4);
            }
            L.b = take(N * 12); L.xr = take((N + 1) / 2 * 12);
            L.flags = take(nb * 4); L.blocks = take(nb * 4); L.tiles = take(nb * 4);
        }
        // the x arrays last and together: level 0's (z), then the coarse ones, which are cleared per extension (a
        // fine cell may read the correction of a coarse cell that is no unknown and sits in a block nobody sweeps)
        lv[0].x = take(N0 * 12);
        xcoarse = off;
        for (int l = 1; l < nlev; ++l)
            lv[l].x = take((size_t)lv[l].w * lv[l].h * 12);
        xcoarse_bytes = off - xcoarse;
        xbest = off;
        if (with_best) take(N0 * 12);
        bytes = off;
    }
};

// The ordered mode's storage of one system, as the host sees it (VmMgbOrd).  The head -- the descriptor, the
// group counts and the group sums of the accumulators the HOST reads (bb, rr[0], rr[1]: the first three) -- is what a
// residual check reads back.
struct MgbOrdLayout {
    int cap, gcap;
    size_t o_ng, o_gpart, head, o_ticket, o_part, bytes;    // offsets from the system's base; head = bytes of a read-back
    MgbOrdLayout(int gx, int gy)
    {
        // producing workgroups of a launch at most: groups of MGB_G = 4 blocks (streaming kernels), tiles of four block rows
        cap = std::max((gx * gy + 3) / 4, gx * ((gy + 3) / 4));
        gcap = (cap + VM_MGB_ORD_GROUP - 1) / VM_MGB_ORD_GROUP;
        o_ng = mgb_align256(sizeof(VmMgbOrd));
        o_gpart = o_ng + mgb_align256(VM_MGB_NACC * sizeof(int));
        head = o_gpart + (size_t)(VM_MGB_ACC_RR + 2) * gcap * 4 * sizeof(double);
        o_ticket = o_gpart + mgb_align256((size_t)VM_MGB_NACC * gcap * 4 * sizeof(double));
        o_part = o_ticket + mgb_align256((size_t)VM_MGB_NACC * gcap * VM_MGB_ORD_TSTRIDE * sizeof(unsigned));
        bytes = o_part + mgb_align256((size_t)VM_MGB_NACC * cap * 4 * sizeof(double));
    }
};

// ---------------------------------------------------------------------------
// The stop test's residual, sqrt(r.r / b.b) of the worst channel, from a read-back (par: the parity r.r was left in);
// -1: a sum is not finite

inline double mgb_rel(const VmMgbScalars &h, int par)
{
    double worst = 0;
    for (int c = 0; c < 3; ++c) {
        double bb = 0, rr = 0;
        for (int k = 0; k < VM_MGB_SLOTS; ++k) { bb += h.bb[k][c]; rr += h.rr[par][k][c]; }
        if (!(bb == bb) || !(rr == rr) || std::isinf(bb) || std::isinf(rr)) return -1;
        if (bb > 0) worst = std::max(worst, std::sqrt(rr / bb));
    }
    return worst;
}

// ... and the stop test's two totals from a read-back head: group sums 0 .. ng - 1 in ascending order from zero
inline double mgb_rel_ordered(const char *head, const MgbOrdLayout &Y, int par)
{
    const int *ng = (const int *)(head + Y.o_ng);
    const double *gp = (const double *)(head + Y.o_gpart);
    auto total = [&](int acc, int c) {
        double t = 0;
        for (int g = 0; g < std::min(ng[acc], Y.gcap); ++g) t += gp[((size_t)acc * Y.gcap + g) * 4 + c];
        return t;
    };
    double worst = 0;
    for (int c = 0; c < 3; ++c) {
        const double bb = total(VM_MGB_ACC_BB, c), rr = total(VM_MGB_ACC_RR + par, c);
        if (!(bb == bb) || !(rr == rr) || std::isinf(bb) || std::isinf(rr)) return -1;
        if (bb > 0) worst = std::max(worst, std::sqrt(rr / bb));
    }
    return worst;
}

// ---------------------------------------------------------------------------
// When a system of a batch is looked at, and when it stops.
// A system's residual is looked at every MGB_LOOK_EVERY iterations (a read drains the stream) until it is within a factor
// MGB_NEAR_TOL of the tolerance -- the cycle gains a decade in two to three iterations -- and every iteration from there:
// a solve stops at the iteration that reaches the tolerance instead of up to three later.  The cadence is the SYSTEM's own
// (next_check): where it stops, and so what it pastes, does not depend on its batch-mates.
#define MGB_LOOK_EVERY 4
#define MGB_NEAR_TOL 30.0
// a system stops when it reaches the tolerance -- or gives up: no better residual for MGB_STALL_ITS iterations, a
// residual MGB_BLOWUP times the best one seen, max_it.  It then holds its best iterate if it kept one, else its
// CURRENT iterate, and reports that iterate's residual (the callers turn a residual above the tolerance into
// VM_E_NUMERIC)
#define MGB_STALL_ITS 12
#define MGB_BLOWUP 1e3

// what MgbStop::observe asks of the driver, or-ed
enum {
    MGB_SAVE_BEST = 1,      // copy the iterate to the room for the best one
    MGB_STOP = 2,           // the system leaves the batch
    MGB_RESTORE_BEST = 4,   // ... with the saved iterate copied back over the current one
    MGB_BREAKDOWN = 8       // a sum was not finite (it == 0: the right-hand side's): the solve fails
};

struct MgbStop {
    double best = 1e300;    // the smallest residual seen; once stopped: the reported one
    int best_it = 0;        // ... and the iteration it was seen after; once stopped: the reported count
    int next_check = 0;
    bool saved = false;

    // is the system looked at after `it` completed iterations?
    bool due(int it) const { return next_check == it; }

    // worst: the residual after `it` completed iterations (mgb_rel / mgb_rel_ordered)
    int observe(int it, double worst, double tol, int max_it, bool has_best_room)
    {
        if (worst < 0) return MGB_BREAKDOWN;
        int verdict = 0;
        if (worst < best) {
            best = worst;
            best_it = it;
            // A system with room for it (the quadratic path: float32 attains 1e-4 .. 1e-5 there, the recursively updated
            // residual passes below what the stored iterate attains and the iteration then drifts) keeps the best
            // iterate seen at a check near the tolerance
            if (has_best_room && worst <= MGB_NEAR_TOL * tol) {
                verdict |= MGB_SAVE_BEST;
                saved = true;
            }
        }
        if (worst <= tol || it >= max_it || it - best_it >= MGB_STALL_ITS || worst > MGB_BLOWUP * best) {
            verdict |= MGB_STOP;
            if (saved && best_it != it) {
                verdict |= MGB_RESTORE_BEST;
            } else {
                best = worst;
                best_it = it;
            }
        }
        next_check = std::min(max_it, it + (best <= MGB_NEAR_TOL * tol ? 1 : MGB_LOOK_EVERY));
        return verdict;
    }
};

// the systems of a batch that are due after `it` iterations lie in [lo, hi]: one read-back of the span that holds them
// (hi < lo: none)
struct MgbSpan {
    int lo, hi;
};

inline MgbSpan mgb_due_span(const std::vector<MgbStop> &stop, uint64_t active, int it)
{
    MgbSpan sp{(int)stop.size(), -1};
    for (int i = 0; i < (int)stop.size(); ++i)
        if (((active >> i) & 1) && stop[i].due(it)) { sp.lo = std::min(sp.lo, i); sp.hi = i; }
    return sp;
}

#endif
