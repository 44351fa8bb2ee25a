// vm_poisson_api.cpp -- C-ABI of the Poisson boundary extension
// (CPoissonExt::run body for one side, Algorithm/PoissonExt.cpp:19-41) and the
// quadratic path of a frame.
#include "vm_host.h"
#include "vm_mgb.h"
#include "vm_poisson.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

namespace {

// grid sizes: halve (rounding up) down to a grid of at most VM_MGB_COARSEST cells
std::vector<std::pair<int, int>> mg_sizes(int w, int h)
{
    std::vector<std::pair<int, int>> v{{w, h}};
    while ((size_t)v.back().first * v.back().second > VM_MGB_COARSEST && (int)v.size() < VM_MGB_MAXLEV)
        v.push_back({(v.back().first + 1) / 2, (v.back().second + 1) / 2});
    return v;
}

// the first level of the cycle's one-workgroup tail: from there on all iterates fit VM_MGB_TAIL_X cells of LDS and all
// right-hand sides but the first VM_MGB_TAIL_B
int mg_tail_level(const std::vector<std::pair<int, int>> &sz)
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

// red-black sweeps each way on level l of the cycle (VmMgbLevel::nu), by kind of system: VM_MGB_NU_POISSON / _QPATH
// (vm_mgb.h: measured choices).  VM_MGB_NU = "a,b,c" overrides both for experiments: sweeps per level from level 0 on, the
// last entry repeats; 1 or 2 on the levels the tile kernels sweep (larger values are cut to 2 there), 1 .. 9 inside the
// one-workgroup tail
int mg_nu(int l, bool in_tail, bool qpath)
{
    static const std::vector<int> env = [] {
        std::vector<int> t;
        if (const char *e = getenv("VM_MGB_NU"))
            for (const char *q = e; *q; ++q)
                if (*q >= '1' && *q <= '9') t.push_back(*q - '0');
        return t;
    }();
    static const std::vector<int> poisson{VM_MGB_NU_POISSON}, path{VM_MGB_NU_QPATH};
    const std::vector<int> &table = !env.empty() ? env : qpath ? path : poisson;
    const int nu = table[std::min((size_t)l, table.size() - 1)];
    return in_tail ? nu : std::min(nu, 2);
}

} // namespace

// ---------------------------------------------------------------------------
// The solver: multigrid-preconditioned CG, batched over systems (a system = one side of one frame), swept over the
// ring of unknowns only, with the fused kernels of vm_mgb.hip.

namespace {

struct MgbWork {          // one system's device workspace, carved from f->pws2[side - 1]
    VmMgbSys S;           // host copy of the device descriptor
    uint8_t *type;
    char *xcoarse;        // the x arrays of levels >= 1, contiguous (cleared per extension)
    size_t xcoarse_bytes;
    VmV3 *Xbest;          // optional (mgb_carve qpath): the iterate with the smallest residual seen near the tolerance
    int *counts;          // nblocks per level, then ntiles per level (device)
    int tail;             // first level of the cycle's one-workgroup tail
    VmV3 *r1;             // second buffer of the PCG residual, for ...
    bool fused;           // ... the PCG update riding in the level-0 restriction (the residual ping-pongs between S.R[0] and S.R[1]):
                          // can this system's hierarchy do it (mgb_carve); whether a solve does: mgb_solve
};

size_t mgb_bytes(int w, int h, bool with_best = false)
{
    const auto sz = mg_sizes(w, h);
    const size_t N0 = (size_t)w * h;
    size_t need = 2 * vm_align256(N0) + vm_align256(sizeof(VmMgbScalars)) + vm_align256(2 * VM_MGB_MAXLEV * sizeof(int)) + 5 * vm_align256(N0 * 12);
    for (size_t l = 0; l < sz.size(); ++l) {
        const size_t N = (size_t)sz[l].first * sz[l].second;
        const size_t nb = (size_t)((sz[l].first + 63) / 64) * ((sz[l].second + 3) / 4);
        need += (l ? 4 * vm_align256(N * 4) : 0) + 2 * vm_align256(N * 12) + vm_align256((N + 1) / 2 * 12) + 3 * vm_align256(nb * 4);
    }
    return need + (with_best ? vm_align256(N0 * 12) : 0);
}

void mgb_carve(MgbWork &W, int w, int h, char *b, bool qpath = false)
{
    const auto sz = mg_sizes(w, h);
    const size_t N0 = (size_t)w * h;
    W.type = (uint8_t *)b; b += vm_align256(N0);
    W.S.type = W.type;
    W.S.sc = (VmMgbScalars *)b; b += vm_align256(sizeof(VmMgbScalars));
    W.counts = (int *)b; b += vm_align256(2 * VM_MGB_MAXLEV * sizeof(int));
    W.tail = mg_tail_level(sz);
    W.S.X = (VmV3 *)b; b += vm_align256(N0 * 12);
    W.S.P[0] = (VmV3 *)b; b += vm_align256(N0 * 12);
    W.S.P[1] = (VmV3 *)b; b += vm_align256(N0 * 12);
    W.S.Q = (VmV3 *)b; b += vm_align256(N0 * 12);
    VmV3 *const r1 = (VmV3 *)b; b += vm_align256(N0 * 12);
    W.S.nlev = (int)sz.size();
    for (size_t l = 0; l < sz.size(); ++l) {
        VmMgbLevel &L = W.S.lv[l];
        L.w = sz[l].first; L.h = sz[l].second;
        L.gx = (L.w + 63) / 64; L.gy = (L.h + 3) / 4;
        const size_t N = (size_t)L.w * L.h, nb = (size_t)L.gx * L.gy;
        L.info = nullptr;
        L.we = L.ws = L.dg = L.k = nullptr;
        if (l == 0) {                       // one byte of operator per cell
            L.info = (uint8_t *)b; b += vm_align256(N);
        } else {
            L.we = (float *)b; b += vm_align256(N * 4);
            L.ws = (float *)b; b += vm_align256(N * 4);
            L.dg = (float *)b; b += vm_align256(N * 4);
            L.k = (float *)b; b += vm_align256(N * 4);
        }
        L.b = (VmV3 *)b; b += vm_align256(N * 12);
        L.nu = mg_nu((int)l, (int)l >= W.tail, qpath);
        L.xr = (VmV3 *)b; b += vm_align256((N + 1) / 2 * 12);
        L.flags = (uint32_t *)b; b += vm_align256(nb * 4);
        L.blocks = (uint32_t *)b; b += vm_align256(nb * 4);
        L.nblocks = W.counts + l;
        L.tiles = (uint32_t *)b; b += vm_align256(nb * 4);
        L.ntiles = W.counts + VM_MGB_MAXLEV + l;
    }
    // the x arrays last and together: level 0's (z), then the coarse ones, which are cleared per extension (a
    // fine cell may read the correction of a coarse cell that is no unknown and sits in a block nobody sweeps)
    W.S.lv[0].x = (VmV3 *)b; b += vm_align256(N0 * 12);
    W.xcoarse = b;
    for (size_t l = 1; l < sz.size(); ++l) {
        W.S.lv[l].x = (VmV3 *)b;
        b += vm_align256((size_t)sz[l].first * sz[l].second * 12);
    }
    W.xcoarse_bytes = (size_t)(b - W.xcoarse);
    W.Xbest = qpath ? (VmV3 *)b : nullptr;     // (the quadratic path keeps the best iterate seen: mgb_solve)
    // The PCG update can ride in the level-0 restriction wherever that kernel exists in its one-sweep form: level 0 swept by
    // the tile kernels (not inside the tail) with one sweep each way
    W.fused = W.tail > 0 && W.S.lv[0].nu == 1;
    W.r1 = r1;
    W.S.R[0] = W.S.R[1] = W.S.lv[0].b;
}

// z = M^-1 r of every active system: one V cycle (sweeps per level: VmMgbLevel::nu); iteration k's r.z lands in rz[k & 1].
// nb / nt: blocks / tiles per level (the largest count among the systems).  In two halves, because the residual norm
// of iteration k - 1 comes out of the FIRST kernel of iteration k when the update rides in the level-0 restriction:
//   mgb_iter_head(k): the PCG update of iteration k - 1 (k >= 1) -- inside the level-0 restriction of cycle k (fused), or
//                     k_mgb_update by itself -- after which x, r and r.r of k completed iterations stand in memory;
//   mgb_iter_rest(k): the rest of cycle k and p = z + beta p, q = A p.
void mgb_iter_head(const VmMgbSys *dev, int nsys, bool fused, const std::vector<int> &nb, const std::vector<int> &nt, int k, uint64_t active,
                   bool ord, hipStream_t s)
{
    if (fused)
        vm_mgb_launch_restrict(dev, nsys, 0, 1, nt[0], k, k > 0, active, ord, s);
    else if (k > 0)
        vm_mgb_launch_update(dev, nsys, nb[0], k - 1, active, ord, s);
}

void mgb_iter_rest(const VmMgbSys *dev, int nsys, const MgbWork &W0, bool fused, const std::vector<int> &nb, const std::vector<int> &nt, int k,
                   uint64_t active, bool ord, hipStream_t s)
{
    const int tail = W0.tail;       // levels tail .. nlev - 1 run in one workgroup
    for (int l = fused ? 1 : 0; l < tail; ++l)
        vm_mgb_launch_restrict(dev, nsys, l, W0.S.lv[l].nu, nt[l], k, false, active, false, s);
    vm_mgb_launch_tail(dev, nsys, tail, active, s);
    if (tail == 0)
        vm_mgb_launch_dot_rz(dev, nsys, nb[0], k, active, ord, s);
    for (int l = tail - 1; l >= 0; --l)
        vm_mgb_launch_prolong(dev, nsys, l, W0.S.lv[l].nu, nt[l], k, active, ord && l == 0, s);
    vm_mgb_launch_dirspmv(dev, nsys, nb[0], k, active, ord, s);
}

double mgb_rel(const VmMgbScalars &h, int par)
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

// The ordered mode's storage of one system, as the host sees it (vm_mgb.h: VmMgbOrd).  The head -- the descriptor, the
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
        o_ng = vm_align256(sizeof(VmMgbOrd));
        o_gpart = o_ng + vm_align256(VM_MGB_NACC * sizeof(int));
        head = o_gpart + (size_t)(VM_MGB_ACC_RR + 2) * gcap * 4 * sizeof(double);
        o_ticket = o_gpart + vm_align256((size_t)VM_MGB_NACC * gcap * 4 * sizeof(double));
        o_part = o_ticket + vm_align256((size_t)VM_MGB_NACC * gcap * VM_MGB_ORD_TSTRIDE * sizeof(unsigned));
        bytes = o_part + vm_align256((size_t)VM_MGB_NACC * cap * 4 * sizeof(double));
    }
};

// ... and the stop test's two totals from a read-back head: group sums 0 .. ng - 1 in ascending order from zero
double mgb_rel_ordered(const char *head, const MgbOrdLayout &Y, int par)
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

} // namespace

// What mgb_setup leaves for the iterations of one batch: where the context keeps the batch's descriptors, scalars and
// ordered-mode storage, and the block / tile counts per level (the largest among the systems)
struct MgbBatch {
    VmMgbSys *dev = nullptr;
    VmMgbScalars *sc_dev = nullptr;
    char *ord_dev = nullptr;
    bool ord = false, fused = false;
    int nlev = 0;
    MgbOrdLayout Y{1, 1};
    std::vector<char> ord_head;        // the systems' descriptors going up, then their read-back heads
    std::vector<int> cnt, nb, nt;      // cnt: every system's counts as mgb_carve lays them out (nblocks, then ntiles per level)
};

// The set-up of a batch: nsys systems of one size whose workspaces are carved and whose type maps are enqueued on the
// context's stream.  Descriptors up, scalars and ordered-mode storage cleared, the hierarchy (level 0, coarsening) and its
// block / tile lists built, their counts read back.
static int mgb_setup(vm_ctx *c, std::vector<MgbWork> &W, int nsys, MgbBatch &B)
{
    hipStream_t s = c->stream;
    if (int rc = c->mgb_sys.reserve(VM_MGB_MAXSYS)) return rc;
    // the systems' PCG scalars and block / tile counts live side by side in one buffer of the context (the descriptors
    // handed to the kernels point there): one clear per solve, one read-back per residual check for the whole batch
    // instead of one per system
    const size_t cnt_bytes = (size_t)VM_MGB_MAXSYS * 2 * VM_MGB_MAXLEV * sizeof(int);
    if (int rc = c->mgb_shared.reserve(VM_MGB_MAXSYS * sizeof(VmMgbScalars) + cnt_bytes)) return rc;
    VmMgbScalars *sc_dev = B.sc_dev = (VmMgbScalars *)c->mgb_shared.get();
    int *cnt_dev = (int *)(c->mgb_shared.get() + VM_MGB_MAXSYS * sizeof(VmMgbScalars));
    VmMgbSys *dev = B.dev = c->mgb_sys.get();
    std::vector<VmMgbSys> hs(nsys);
    const int nlev = B.nlev = W[0].S.nlev;
    // VM_REDUCE_ORDERED: every system's partials, tickets and group sums, from the context like the scalars; the descriptors,
    // group counts and tickets are cleared once per solve (a launch leaves its tickets at zero again)
    const bool ord = B.ord = c->reduction == VM_REDUCE_ORDERED;
    const MgbOrdLayout Y = B.Y = MgbOrdLayout(W[0].S.lv[0].gx, W[0].S.lv[0].gy);
    char *ord_dev = nullptr;
    if (ord) {
        if (int rc = c->mgb_ord.reserve((size_t)nsys * Y.bytes)) return rc;
        ord_dev = B.ord_dev = c->mgb_ord.get();
    }
    // The PCG update rides in the level-0 restriction wherever the hierarchy allows it.  Measured on the 2304 x 1464 canvas
    // (tools/exp/fuse_ab.sh, ms per frame at 1e-5, fused against the separate k_mgb_update): 8 systems per batch 1.61 / 1.70,
    // 4 systems 1.95 / 1.99, 2 systems 2.49 / 2.51, one system 1.78 / 1.81 per side (with the fused kernel's loads issued cell
    // by cell it lost on one and two systems, 2.56 / 2.49: vm_mgb.hip).  Same arithmetic either way.
    // VM_MGB_FUSE_MIN_SYS (dev switch): the smallest batch that fuses (0: never).
    static const int fuse_min = [] { const char *e = getenv("VM_MGB_FUSE_MIN_SYS"); return e ? atoi(e) : 1; }();
    const bool fused = B.fused = W[0].fused && fuse_min > 0 && nsys >= fuse_min;
    for (int i = 0; i < nsys; ++i) {
        W[i].S.R[1] = fused ? W[i].r1 : W[i].S.R[0];
        hs[i] = W[i].S;
        hs[i].sc = sc_dev + i;
        if (ord) hs[i].ord = (const VmMgbOrd *)(ord_dev + (size_t)i * Y.bytes);
        for (int l = 0; l < nlev; ++l) {
            hs[i].lv[l].nblocks = cnt_dev + (size_t)i * 2 * VM_MGB_MAXLEV + l;
            hs[i].lv[l].ntiles = cnt_dev + (size_t)i * 2 * VM_MGB_MAXLEV + VM_MGB_MAXLEV + l;
        }
    }
    VM_HIP(hipMemcpyAsync(dev, hs.data(), nsys * sizeof(VmMgbSys), hipMemcpyHostToDevice, s));
    VM_HIP(hipMemsetAsync(sc_dev, 0, nsys * sizeof(VmMgbScalars), s));
    std::vector<char> &ord_head = B.ord_head;
    if (ord) {
        ord_head.assign((size_t)nsys * Y.head, 0);
        for (int i = 0; i < nsys; ++i) {
            char *base = ord_dev + (size_t)i * Y.bytes;
            VM_HIP(hipMemsetAsync(base, 0, Y.o_part, s));
            const VmMgbOrd d{Y.cap, Y.gcap, (double *)(base + Y.o_part), (double *)(base + Y.o_gpart), (unsigned *)(base + Y.o_ticket), (int *)(base + Y.o_ng)};
            memcpy(&ord_head[(size_t)i * Y.head], &d, sizeof(d));
            VM_HIP(hipMemcpyAsync(base, &ord_head[(size_t)i * Y.head], sizeof(d), hipMemcpyHostToDevice, s));
        }
    }
    for (int i = 0; i < nsys; ++i)
        if (W[i].xcoarse_bytes) VM_HIP(hipMemsetAsync(W[i].xcoarse, 0, W[i].xcoarse_bytes, s));
    // the hierarchy and its block lists (batched)
    vm_mgb_launch_level0(dev, nsys, W[0].S.lv[0].gx, W[0].S.lv[0].gy, s);
    for (int l = 1; l < nlev; ++l)
        vm_mgb_launch_coarsen(dev, nsys, l, W[0].S.lv[l].gx, W[0].S.lv[l].gy, s);
    vm_mgb_launch_compact(dev, nsys, nlev, s);
    VM_HIP(hipGetLastError());
    std::vector<int> &cnt = B.cnt, &nb = B.nb, &nt = B.nt;
    cnt.assign((size_t)nsys * 2 * VM_MGB_MAXLEV, 0);
    nb.assign(nlev, 0);
    nt.assign(nlev, 0);
    VM_HIP(hipMemcpyAsync(cnt.data(), cnt_dev, (size_t)nsys * 2 * VM_MGB_MAXLEV * sizeof(int), hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < nsys; ++i)
        for (int l = 0; l < nlev; ++l) {
            nb[l] = std::max(nb[l], cnt[(size_t)i * 2 * VM_MGB_MAXLEV + l]);
            nt[l] = std::max(nt[l], cnt[(size_t)i * 2 * VM_MGB_MAXLEV + VM_MGB_MAXLEV + l]);
        }
    return VM_OK;
}

// The batched PCG proper: nsys systems of one size whose workspaces are carved, whose type maps, right-hand sides
// (lv[0].b) and initial guesses (X) are enqueued on the context's stream.  Leaves every system's solution in its X
// (the iterate it stopped at; the best one seen near the tolerance if the workspace was carved with room for it), its
// iteration count and relative residual in iters / rels.
static int mgb_solve(vm_ctx *c, std::vector<MgbWork> &W, int nsys, float tol, int max_it, int *iters, double *rels)
{
    hipStream_t s = c->stream;
    const size_t N0 = (size_t)W[0].S.lv[0].w * W[0].S.lv[0].h;
    MgbBatch B;
    if (int rc = mgb_setup(c, W, nsys, B)) return rc;
    VmMgbSys *const dev = B.dev;
    VmMgbScalars *const sc_dev = B.sc_dev;
    char *const ord_dev = B.ord_dev;
    const bool ord = B.ord, fused = B.fused;
    const MgbOrdLayout &Y = B.Y;
    std::vector<char> &ord_head = B.ord_head;
    const std::vector<int> &nb = B.nb, &nt = B.nt;
    if (nb[0] == 0) {                       // no unknown anywhere: nothing to extend
        for (int i = 0; i < nsys; ++i) { iters[i] = 0; rels[i] = 0; }
        return VM_OK;
    }
    uint64_t active = nsys == 64 ? ~0ull : ((1ull << nsys) - 1);
    vm_mgb_launch_init(dev, nsys, nb[0], active, ord, s);
    std::vector<VmMgbScalars> h(nsys);
    std::vector<double> best(nsys, 1e300);
    std::vector<int> best_it(nsys, 0), next_check(nsys, 0), saved(nsys, 0);
    std::vector<std::pair<VmEvent, VmEvent>> prof_ev;
    std::vector<int> prof_sys;
    int it = 0;
    // A system's residual is looked at every 4 iterations (a read drains the stream) until it is within a factor 30
    // of the tolerance -- the cycle gains a decade in two to three iterations -- and every iteration from there: a solve
    // stops at the iteration that reaches the tolerance instead of up to three later.  The cadence is the SYSTEM's own
    // (next_check): where it stops, and so what it pastes, does not depend on its batch-mates.
    // check(it): the systems due after `it` completed iterations (mgb_iter_head(it) has been enqueued: x, r, r.r are theirs)
    auto check = [&](int it) -> int {
        int lo = nsys, hi = -1;          // the systems looked at now: one read-back of the span that holds them
        for (int i = 0; i < nsys; ++i)
            if (((active >> i) & 1) && next_check[i] == it) { lo = std::min(lo, i); hi = i; }
        if (hi < lo) return VM_OK;
        if (ord)
            VM_HIP(hipMemcpy2DAsync(&ord_head[(size_t)lo * Y.head], Y.head, ord_dev + (size_t)lo * Y.bytes, Y.bytes, Y.head, (size_t)(hi - lo + 1),
                                    hipMemcpyDeviceToHost, s));
        else
            VM_HIP(hipMemcpyAsync(&h[lo], sc_dev + lo, (size_t)(hi - lo + 1) * sizeof(VmMgbScalars), hipMemcpyDeviceToHost, s));
        VM_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nsys; ++i) {
            if (!((active >> i) & 1) || next_check[i] != it) continue;
            // it == 0: parity 1, where k_mgb_init left r.r
            const double worst = ord ? mgb_rel_ordered(&ord_head[(size_t)i * Y.head], Y, (it - 1) & 1) : mgb_rel(h[i], (it - 1) & 1);
            if (worst < 0)
                return vm_fail(VM_E_NUMERIC, it == 0 ? "multigrid PCG: the right-hand side is not finite" : "multigrid PCG broke down (NaN)");
            if (worst < best[i]) {
                best[i] = worst;
                best_it[i] = it;
                // A system with room for it (the quadratic path: float32 attains 1e-4 .. 1e-5 there, the recursively updated
                // residual passes below what the stored iterate attains and the iteration then drifts) keeps the best
                // iterate seen at a check near the tolerance
                if (W[i].Xbest && worst <= 30.0 * tol) {
                    VM_HIP(hipMemcpyAsync(W[i].Xbest, W[i].S.X, N0 * sizeof(VmV3), hipMemcpyDeviceToDevice, s));
                    saved[i] = 1;
                }
            }
            // a system stops when it reaches the tolerance -- or gives up: no better residual for 12 iterations, a
            // residual 1000 times the best one seen, max_it.  It then holds its best iterate if it kept one, else its
            // CURRENT iterate, and reports that iterate's residual (the callers turn a residual above the tolerance into
            // VM_E_NUMERIC)
            if (worst <= tol || it >= max_it || it - best_it[i] >= 12 || worst > 1e3 * best[i]) {
                active &= ~(1ull << i);
                if (saved[i] && best_it[i] != it) {
                    VM_HIP(hipMemcpyAsync(W[i].S.X, W[i].Xbest, N0 * sizeof(VmV3), hipMemcpyDeviceToDevice, s));
                } else {
                    best[i] = worst;
                    best_it[i] = it;
                }
            }
            next_check[i] = std::min(max_it, it + (best[i] <= 30.0 * tol ? 1 : 4));
        }
        return VM_OK;
    };
    {
        const int rc = check(0);
        if (rc != VM_OK) return rc;
    }
    while (active) {
        if (c->mgb_prof && it > 0) {     // the probe of vm_dbg_poisson_profile: events around the launch that carries the update
            prof_ev.emplace_back();
            VmEvent &e0 = prof_ev.back().first, &e1 = prof_ev.back().second;
            if (int rc = e0.create()) return rc;
            if (int rc = e1.create()) return rc;
            VM_HIP(hipEventRecord(e0.get(), s));
            mgb_iter_head(dev, nsys, fused, nb, nt, it, active, ord, s);
            VM_HIP(hipEventRecord(e1.get(), s));
            prof_sys.push_back(__builtin_popcountll(active));
        } else {
            mgb_iter_head(dev, nsys, fused, nb, nt, it, active, ord, s);
        }
        if (it > 0) {
            const int rc = check(it);
            if (rc != VM_OK) return rc;
            if (!active) break;
        }
        mgb_iter_rest(dev, nsys, W[0], fused, nb, nt, it, active, ord, s);
        ++it;
        VM_HIP(hipGetLastError());
    }
    for (int i = 0; i < nsys; ++i) {
        iters[i] = best_it[i];
        rels[i] = best[i];
    }
    if (!prof_ev.empty()) {
        VM_HIP(hipStreamSynchronize(s));
        for (size_t k = 0; k < prof_ev.size(); ++k) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, prof_ev[k].first.get(), prof_ev[k].second.get()) == hipSuccess) {
                c->mgb_prof_us += 1e3 * ms;
                c->mgb_prof_launches += 1;
                c->mgb_prof_fused += fused ? 1 : 0;
                c->mgb_prof_unknown_launches += prof_sys[k];        // active systems of that launch (x unknowns per system: the caller's)
            }
        }
    }
    return VM_OK;
}

// Diagnostic (bench.py's roofline of the compositor's HBM-bound kernel, measured live as the contract asks: HIP events on
// the stream the kernel is launched on): on != 0 arms the probe and clears its sums; on == 0 disarms it and returns the
// HIP-event time of the launches that carried the PCG update since (microseconds, summed), their number, the number of
// ACTIVE systems summed over those launches, and how many of them were the level-0 restriction with the update fused in
// (k_mgb_restrict<true, true>: 76 B per unknown of every active system) rather than k_mgb_update by itself (73 B).
extern "C" int vm_dbg_poisson_profile(vm_ctx *c, int on, double *update_us, int *update_launches, double *active_systems, int *fused_launches)
{
    if (!c) return vm_fail(VM_E_INVALID, "vm_dbg_poisson_profile: ctx is NULL");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (on) {
        c->mgb_prof = true;
        c->mgb_prof_us = c->mgb_prof_unknown_launches = 0;
        c->mgb_prof_launches = c->mgb_prof_fused = 0;
        return VM_OK;
    }
    c->mgb_prof = false;
    if (update_us) *update_us = c->mgb_prof_us;
    if (update_launches) *update_launches = c->mgb_prof_launches;
    if (active_systems) *active_systems = c->mgb_prof_unknown_launches;
    if (fused_launches) *fused_launches = c->mgb_prof_fused;
    return VM_OK;
}

// One system's workspace and type map, enqueued: `which` = side 1 or 2 of the frame's Poisson extension (the canvas classified;
// fill: and its outside pixels filled from the other image, vm_poisson_launch_prepare -- what a solve needs for its right-hand
// side) or VM_DBG_MGB_QPATH, the quadratic path's whole-grid system (every pixel an unknown without a tie: type 2 everywhere,
// so the level-0 operator is the graph Laplacian of the pixel grid with Neumann ends, QuadraticPath.cpp:137-170; the workspace
// is side 1's of the Poisson extension: the frame is no larger than its canvas, the two run in turn)
static int mgb_system(vm_frame *f, int which, MgbWork &W, bool fill)
{
    hipStream_t s = f->ctx->stream;
    if (which == VM_DBG_MGB_QPATH) {
        int rc = f->pws2[0].reserve(std::max(mgb_bytes(std::max(f->w, f->cw), std::max(f->h, f->ch)), mgb_bytes(f->w, f->h, true)));
        if (rc != VM_OK) return rc;
        mgb_carve(W, f->w, f->h, f->pws2[0].get(), true);
        VM_HIP(hipMemsetAsync(W.type, 2, (size_t)f->w * f->h, s));
        return VM_OK;
    }
    const int side = which;
    if (int rc = f->pws2[side - 1].reserve(mgb_bytes(f->cw, f->ch))) return rc;
    mgb_carve(W, f->cw, f->ch, f->pws2[side - 1].get());
    uchar4 *ext = f->ext[side - 1].get();
    if (fill) {
        const uchar4 *other = f->crop[side == 1 ? 1 : 0].get(); // PoissonExt.cpp:54-57
        vm_poisson_launch_prepare(ext, W.type, other, f->v.get(), f->w, f->h, f->rs, f->ex, side == 1 ? 1 : -1, s);
    } else {
        vm_poisson_launch_classify(ext, W.type, f->cw, f->ch, s);
    }
    return VM_OK;
}

// Poisson extension of nsys systems (frames[i], sides[i]) of one context and one canvas size as ONE batch
static int poisson_solve_batch(vm_ctx *c, vm_frame *const *frames, const int *sides, int nsys, float tol, int max_it,
                               int *iters, double *rels)
{
    hipStream_t s = c->stream;
    const int cw = frames[0]->cw, ch = frames[0]->ch;
    std::vector<MgbWork> W(nsys);
    // classify, fill, right-hand side + initial guess (per system)
    for (int i = 0; i < nsys; ++i) {
        vm_frame *f = frames[i];
        const int side = sides[i];
        if (int rc = mgb_system(f, side, W[i], true)) return rc;
        vm_poisson_launch_setup3(f->ext[side - 1].get(), W[i].type, W[i].S.lv[0].b, W[i].S.X, cw, ch, s);
    }
    int rc = mgb_solve(c, W, nsys, tol, max_it, iters, rels);
    if (rc != VM_OK) return rc;
    for (int i = 0; i < nsys; ++i)
        vm_poisson_launch_paste3(frames[i]->ext[sides[i] - 1].get(), W[i].type, W[i].S.X, cw, ch, s);
    VM_HIP(hipGetLastError());
    return VM_OK;
}

extern "C" int vm_poisson_extend(vm_frame *f, int side, float tol, int max_it, int *iters,
                                 float *rel_res, float *elapsed_ms)
{
    if ((side != 1 && side != 2) || !(tol > 0) || max_it < 1)
        return vm_fail(VM_E_INVALID, "vm_poisson_extend: bad argument");
    VM_ENTER_LOCKED(f);
    vm_ctx *c = f->ctx;
    hipStream_t s = c->stream;
    VM_HIP(hipEventRecord(c->ev0.get(), s));
    int total_it = 0;
    double rel = 0;
    int rc = poisson_solve_batch(c, &f, &side, 1, tol, max_it, &total_it, &rel);
    if (rc != VM_OK) return rc;
    VM_HIP(hipGetLastError());
    VM_HIP(hipEventRecord(c->ev1.get(), s));
    VM_HIP(hipEventSynchronize(c->ev1.get()));
    float ms = 0;
    VM_HIP(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()));
    if (iters) *iters = total_it;
    if (rel_res) *rel_res = (float)rel;
    if (elapsed_ms) *elapsed_ms = ms;
    if (rel > tol)
        return vm_fail(VM_E_NUMERIC, "vm_poisson_extend: residual %.3g after %d iterations (tol %.3g)", rel, total_it, (double)tol);
    return VM_OK;
}

// Both sides of n frames in one batch: CPoissonExt::run's loop body (PoissonExt.cpp:24-36) for n frames at once --
// side 1 samples the ORIGINAL image 2 and side 2 the original image 1 (the crops taken at upload), so the 2 n
// systems are independent.  iters / rel_res: 2 n entries, [2 i] = side 1 of frame i, [2 i + 1] = side 2.
extern "C" int vm_poisson_extend_frames(vm_frame *const *frames, int n, float tol, int max_it, int *iters,
                                        float *rel_res, float *elapsed_ms)
{
    if (!frames || n < 1 || 2 * n > VM_MGB_MAXSYS || !(tol > 0) || max_it < 1)
        return vm_fail(VM_E_INVALID, "vm_poisson_extend_frames: bad argument (1 <= n <= %d)", VM_MGB_MAXSYS / 2);
    for (int i = 0; i < n; ++i) {
        if (!frames[i]) return vm_fail(VM_E_INVALID, "vm_poisson_extend_frames: frame %d is NULL", i);
        if (frames[i]->ctx != frames[0]->ctx) return vm_fail(VM_E_INVALID, "vm_poisson_extend_frames: the frames belong to different contexts");
        if (frames[i]->cw != frames[0]->cw || frames[i]->ch != frames[0]->ch)
            return vm_fail(VM_E_INVALID, "vm_poisson_extend_frames: the frames differ in size");
        for (int j = 0; j < i; ++j)
            if (frames[j] == frames[i]) return vm_fail(VM_E_INVALID, "vm_poisson_extend_frames: frame %d listed twice", i);
    }
    VM_ENTER_LOCKED(frames[0]);
    vm_ctx *c = frames[0]->ctx;
    hipStream_t s = c->stream;
    std::vector<vm_frame *> fr(2 * n);
    std::vector<int> sd(2 * n), its(2 * n, 0);
    std::vector<double> rel(2 * n, 0.0);
    for (int i = 0; i < n; ++i) { fr[2 * i] = fr[2 * i + 1] = frames[i]; sd[2 * i] = 1; sd[2 * i + 1] = 2; }
    VM_HIP(hipEventRecord(c->ev0.get(), s));
    int rc = poisson_solve_batch(c, fr.data(), sd.data(), 2 * n, tol, max_it, its.data(), rel.data());
    if (rc != VM_OK) return rc;
    VM_HIP(hipEventRecord(c->ev1.get(), s));
    VM_HIP(hipEventSynchronize(c->ev1.get()));
    float ms = 0;
    VM_HIP(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()));
    if (elapsed_ms) *elapsed_ms = ms;
    double worst = 0;
    int at = 0;
    for (int i = 0; i < 2 * n; ++i) {
        if (iters) iters[i] = its[i];
        if (rel_res) rel_res[i] = (float)rel[i];
        if (rel[i] > worst) { worst = rel[i]; at = i; }
    }
    if (worst > tol)
        return vm_fail(VM_E_NUMERIC, "vm_poisson_extend_frames: residual %.3g after %d iterations on side %d of frame %d (tol %.3g)",
                       worst, its[at], at % 2 + 1, at / 2, (double)tol);
    return VM_OK;
}

// ---------------------------------------------------------------------------
// Read-only views of the preconditioner for the tests (include/vmorph.h: vm_dbg_mgb_*): the production set-up (mgb_system,
// mgb_setup) and the production cycle (mgb_iter_head / mgb_iter_rest) on the production workspace, and downloads.

namespace {

// the hierarchy of system `which` of the frame, built as a solve of ONE system would build it -- but from the canvas as it
// stands: classified, not filled
int mgb_dbg_build(vm_frame *f, int which, const char *fn, std::vector<MgbWork> &W, MgbBatch &B)
{
    if (which != 1 && which != 2 && which != VM_DBG_MGB_QPATH)
        return vm_fail(VM_E_INVALID, "%s: which must be 1, 2 or VM_DBG_MGB_QPATH", fn);
    if (which == VM_DBG_MGB_QPATH && (f->w < 2 || f->h < 2))
        return vm_fail(VM_E_INVALID, "%s: the quadratic path needs a frame of at least 2x2 pixels", fn);
    W.resize(1);
    if (int rc = mgb_system(f, which, W[0], false)) return rc;
    return mgb_setup(f->ctx, W, 1, B);
}

int mgb_dbg_download(void *host, const void *dev, size_t bytes, hipStream_t s)
{
    if (host) VM_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    return VM_OK;
}

} // namespace

extern "C" int vm_dbg_mgb_setup(vm_frame *f, int which, int *nlev, int *tail, int *w, int *h, int *nu, int *nblocks, int *ntiles)
{
    VM_ENTER_LOCKED(f);
    std::vector<MgbWork> W;
    MgbBatch B;
    if (int rc = mgb_dbg_build(f, which, __func__, W, B)) return rc;
    if (nlev) *nlev = B.nlev;
    if (tail) *tail = W[0].tail;
    for (int l = 0; l < B.nlev; ++l) {
        if (w) w[l] = W[0].S.lv[l].w;
        if (h) h[l] = W[0].S.lv[l].h;
        if (nu) nu[l] = W[0].S.lv[l].nu;
        if (nblocks) nblocks[l] = B.cnt[l];
        if (ntiles) ntiles[l] = B.cnt[VM_MGB_MAXLEV + l];
    }
    return VM_OK;
}

extern "C" int vm_dbg_mgb_level(vm_frame *f, int which, int l, float *dg, float *we, float *ws, float *b, float *x, int *have)
{
    VM_ENTER_LOCKED(f);
    if (which != 1 && which != 2 && which != VM_DBG_MGB_QPATH)
        return vm_fail(VM_E_INVALID, "vm_dbg_mgb_level: which must be 1, 2 or VM_DBG_MGB_QPATH");
    const bool qpath = which == VM_DBG_MGB_QPATH;
    const int gw = qpath ? f->w : f->cw, gh = qpath ? f->h : f->ch;
    VmDev<char> &ws_buf = f->pws2[qpath ? 0 : which - 1];
    if (!ws_buf.get() || ws_buf.capacity() < mgb_bytes(gw, gh, qpath))
        return vm_fail(VM_E_STATE, "vm_dbg_mgb_level: no hierarchy in the frame (vm_dbg_mgb_setup or vm_dbg_mgb_cycle first)");
    MgbWork W;
    mgb_carve(W, gw, gh, ws_buf.get(), qpath);       // where the set-up put things: pointers only, nothing is launched
    if (l < 0 || l >= W.S.nlev)
        return vm_fail(VM_E_INVALID, "vm_dbg_mgb_level: level %d of %d", l, W.S.nlev);
    hipStream_t s = f->ctx->stream;
    const VmMgbLevel &L = W.S.lv[l];
    const size_t N = (size_t)L.w * L.h;
    std::vector<uint8_t> info;
    if (l == 0) {
        info.resize(N);
        if (int rc = mgb_dbg_download(info.data(), L.info, N, s)) return rc;
    } else {
        if (int rc = mgb_dbg_download(dg, L.dg, N * 4, s)) return rc;
        if (int rc = mgb_dbg_download(we, L.we, N * 4, s)) return rc;
        if (int rc = mgb_dbg_download(ws, L.ws, N * 4, s)) return rc;
    }
    // a level's right-hand side and result stand in memory down to the first level of the tail (the tail keeps the rest in LDS)
    const bool in_memory = l <= W.tail;
    if (in_memory) {
        if (int rc = mgb_dbg_download(b, L.b, N * sizeof(VmV3), s)) return rc;
        if (int rc = mgb_dbg_download(x, L.x, N * sizeof(VmV3), s)) return rc;
    }
    VM_HIP(hipStreamSynchronize(s));
    if (l == 0)                                      // the info byte, decoded (vm_mgb.h)
        for (size_t i = 0; i < N; ++i) {
            if (dg) dg[i] = (float)(info[i] >> 4);
            if (we) we[i] = (float)(info[i] & 1u);
            if (ws) ws[i] = (float)((info[i] >> 2) & 1u);
        }
    if (have) *have = in_memory ? 3 : 0;
    return VM_OK;
}

extern "C" int vm_dbg_mgb_cycle(vm_frame *f, int which, const float *r_in, float *z_out, float *q_out)
{
    if (!r_in) return vm_fail(VM_E_INVALID, "vm_dbg_mgb_cycle: r_in is NULL");
    VM_ENTER_LOCKED(f);
    vm_ctx *c = f->ctx;
    hipStream_t s = c->stream;
    std::vector<MgbWork> W;
    MgbBatch B;
    if (int rc = mgb_dbg_build(f, which, __func__, W, B)) return rc;
    const VmMgbLevel &L = W[0].S.lv[0];
    const size_t N0 = (size_t)L.w * L.h;
    if (B.nb[0] == 0) {                              // no unknown: M^-1 of nothing
        if (z_out) memset(z_out, 0, N0 * sizeof(VmV3));
        if (q_out) memset(q_out, 0, N0 * sizeof(VmV3));
        return VM_OK;
    }
    VM_HIP(hipMemcpyAsync(L.b, r_in, N0 * sizeof(VmV3), hipMemcpyHostToDevice, s));      // the residual of iteration 0: R[0]
    mgb_iter_head(B.dev, 1, B.fused, B.nb, B.nt, 0, 1ull, B.ord, s);
    mgb_iter_rest(B.dev, 1, W[0], B.fused, B.nb, B.nt, 0, 1ull, B.ord, s);
    VM_HIP(hipGetLastError());
    std::vector<uint8_t> info(N0);
    if (int rc = mgb_dbg_download(info.data(), L.info, N0, s)) return rc;
    if (int rc = mgb_dbg_download(z_out, L.x, N0 * sizeof(VmV3), s)) return rc;
    if (int rc = mgb_dbg_download(q_out, W[0].S.Q, N0 * sizeof(VmV3), s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    // cells without an unknown outside every swept tile / block are memory nobody wrote: zeros in what is handed out
    for (size_t i = 0; i < N0; ++i)
        if ((info[i] >> 4) == 0)
            for (int ch = 0; ch < 3; ++ch) {
                if (z_out) z_out[3 * i + ch] = 0;
                if (q_out) q_out[3 * i + ch] = 0;
            }
    return VM_OK;
}

// CQuadraticPath::optimize for the frame's halfway field (QuadraticPath.cpp:24-223): u goes
// to the frame's quadratic-path buffer, where vm_render_halfway reads it
extern "C" int vm_frame_quadratic_path(vm_frame *f, float tol, int max_it, int *iters, float *rel_res,
                                       float *elapsed_ms)
{
    if (!(tol > 0) || max_it < 1)
        return vm_fail(VM_E_INVALID, "vm_frame_quadratic_path: bad argument");
    VM_ENTER_LOCKED(f);
    if (f->w < 2 || f->h < 2)
        return vm_fail(VM_E_INVALID, "vm_frame_quadratic_path: needs a frame of at least 2x2 pixels");
    vm_ctx *c = f->ctx;
    hipStream_t s = c->stream;
    int it = 0;
    double rel = 0;
    VM_HIP(hipEventRecord(c->ev0.get(), s));
    {
        // the batched solver on the whole grid (mgb_system)
        std::vector<MgbWork> W(1);
        int rc = mgb_system(f, VM_DBG_MGB_QPATH, W[0], false);
        if (rc != VM_OK) return rc;
        vm_qpath_launch_rhs3(f->v.get(), f->rs, f->w, f->h, W[0].S.lv[0].b, W[0].S.X, s);
        // project the right-hand side onto the range of the singular operator
        double *sums = &W[0].S.sc->bb[0][0];
        // VM_REDUCE_ORDERED: the sums' workgroup partials go through scratch of the workspace -- Q, which the solve writes
        // before it reads and nobody reads after it (16 bytes per 64 x 4-cell block at most, of 12 per cell of a field >= 2 x 2)
        double *const ord_part = c->reduction == VM_REDUCE_ORDERED ? (double *)W[0].S.Q : nullptr;
        VM_HIP(hipMemsetAsync(W[0].S.sc, 0, sizeof(VmMgbScalars), s));
        vm_qpath_launch_sum3(W[0].S.lv[0].b, f->w, f->h, sums, ord_part, s);
        vm_qpath_launch_shift3(W[0].S.lv[0].b, f->w, f->h, sums, nullptr, 0, s);
        VM_HIP(hipGetLastError());
        rc = mgb_solve(c, W, 1, tol, max_it, &it, &rel);
        if (rc != VM_OK) return rc;
        VM_HIP(hipMemsetAsync(W[0].S.sc, 0, sizeof(VmMgbScalars), s));
        vm_qpath_launch_sum3(W[0].S.X, f->w, f->h, sums, ord_part, s);
        vm_qpath_launch_shift3(W[0].S.X, f->w, f->h, sums, f->u.get(), f->rs, s);
    }
    f->u_zero = false;
    VM_HIP(hipGetLastError());
    VM_HIP(hipEventRecord(c->ev1.get(), s));
    VM_HIP(hipEventSynchronize(c->ev1.get()));
    float ms = 0;
    VM_HIP(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()));
    if (iters) *iters = it;
    if (rel_res) *rel_res = (float)rel;
    if (elapsed_ms) *elapsed_ms = ms;
    if (rel > tol)
        return vm_fail(VM_E_NUMERIC, "vm_frame_quadratic_path: residual %.3g after %d iterations (tol %.3g)", rel, it, (double)tol);
    return VM_OK;
}

// the frame's quadratic path, tight (h, w, 2) floats
extern "C" int vm_frame_download_qpath(vm_frame *f, float *u_xy)
{
    if (!u_xy) return vm_fail(VM_E_INVALID, "vm_frame_download_qpath: bad argument");
    VM_ENTER(f);
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->u.get(), (size_t)f->rs * 8, u_xy, 0, 8, (size_t)f->w * 8, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

// the frame's halfway field as the compositor holds it, tight (h, w, 2) floats (_vector[frame] of
// the reference's Pyramid once update_result has run)
extern "C" int vm_frame_download_v(vm_frame *f, float *v_xy)
{
    if (!v_xy) return vm_fail(VM_E_INVALID, "vm_frame_download_v: bad argument");
    VM_ENTER(f);
    hipStream_t s = f->ctx->stream;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->v.get(), (size_t)f->rs * 8, v_xy, 0, 8, (size_t)f->w * 8, f->h, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}
