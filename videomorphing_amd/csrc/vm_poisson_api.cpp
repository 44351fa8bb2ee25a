// vm_poisson_api.cpp -- C-ABI of the Poisson boundary extension
// (CPoissonExt::run body for one side, Algorithm/PoissonExt.cpp:19-41) and the
// quadratic path of a frame.  The launcher of the batched solver: its rules -- hierarchy, workspace layout, host folds,
// stop rule -- are vm_mgb_plan.h's.
#include "vm_host.h"
#include "vm_mgb.h"
#include "vm_poisson.h"
#include "vm_layer_ext.h"

#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

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
    int tail;             // first level of the cycle's one-workgroup tail
    VmV3 *r1;             // second buffer of the PCG residual, for the PCG update riding in the level-0 restriction (the
                          // residual ping-pongs between S.R[0] and S.R[1]); whether a solve does: mgb_setup
};

size_t mgb_bytes(int w, int h, bool with_best = false) { return MgbLayout(w, h, with_best).bytes; }

// pointers into a workspace at b, by the layout; qpath: the quadratic path's system (its sweeps per level, and room for the
// best iterate)
void mgb_carve(MgbWork &W, int w, int h, char *b, bool qpath = false)
{
    const MgbLayout A(w, h, qpath);
    const std::vector<int> &nu = mg_nu_table(MgbSwitches::from_environment(), qpath);
    auto at = [b](auto *&p, size_t off) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(b + off); };
    int *counts;        // nblocks per level, then ntiles per level (device)
    at(W.type, A.type); at(W.S.sc, A.sc); at(counts, A.counts);
    at(W.S.X, A.X); at(W.S.P[0], A.P[0]); at(W.S.P[1], A.P[1]); at(W.S.Q, A.Q); at(W.r1, A.r1);
    W.S.type = W.type;
    W.tail = A.tail;
    W.S.nlev = A.nlev;
    for (int l = 0; l < A.nlev; ++l) {
        const MgbLevelLayout &O = A.lv[l];
        VmMgbLevel &L = W.S.lv[l];
        L.w = O.w; L.h = O.h;
        L.gx = O.gx; L.gy = O.gy;
        L.info = nullptr;
        L.we = L.ws = L.dg = L.k = nullptr;
        if (l == 0) {                       // one byte of operator per cell
            at(L.info, O.info);
        } else {
            at(L.we, O.we); at(L.ws, O.ws); at(L.dg, O.dg); at(L.k, O.k);
        }
        at(L.b, O.b); at(L.xr, O.xr); at(L.x, O.x);
        at(L.flags, O.flags); at(L.blocks, O.blocks); at(L.tiles, O.tiles);
        L.nu = mg_nu(nu, l, l >= A.tail);
        L.nblocks = counts + l;
        L.ntiles = counts + VM_MGB_MAXLEV + l;
    }
    at(W.xcoarse, A.xcoarse);
    W.xcoarse_bytes = A.xcoarse_bytes;
    W.Xbest = nullptr;
    if (qpath) at(W.Xbest, A.xbest);       // (the quadratic path keeps the best iterate seen: MgbStop)
    W.S.R[0] = W.S.R[1] = W.S.lv[0].b;
}

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
    std::vector<VmMgbScalars> sc_host; // ... and the read-back scalars of the default mode (mgb_look)
    std::vector<int> cnt, nb, nt;      // cnt: every system's counts as mgb_carve lays them out (nblocks, then ntiles per level)
};

// z = M^-1 r of every active system: one V cycle (sweeps per level: VmMgbLevel::nu); iteration k's r.z lands in rz[k & 1].
// B.nb / nt: blocks / tiles per level (the largest count among the systems).  In two halves, because the residual norm
// of iteration k - 1 comes out of the FIRST kernel of iteration k when the update rides in the level-0 restriction:
//   mgb_iter_head(k): the PCG update of iteration k - 1 (k >= 1) -- inside the level-0 restriction of cycle k (fused), or
//                     k_mgb_update by itself -- after which x, r and r.r of k completed iterations stand in memory;
//   mgb_iter_rest(k): the rest of cycle k and p = z + beta p, q = A p.
void mgb_iter_head(const MgbBatch &B, int nsys, int k, uint64_t active, hipStream_t s)
{
    if (B.fused)
        vm_mgb_launch_restrict(B.dev, nsys, 0, 1, B.nt[0], k, k > 0, active, B.ord, s);
    else if (k > 0)
        vm_mgb_launch_update(B.dev, nsys, B.nb[0], k - 1, active, B.ord, s);
}

void mgb_iter_rest(const MgbBatch &B, int nsys, const MgbWork &W0, int k, uint64_t active, hipStream_t s)
{
    const int tail = W0.tail;       // levels tail .. nlev - 1 run in one workgroup
    for (int l = B.fused ? 1 : 0; l < tail; ++l)
        vm_mgb_launch_restrict(B.dev, nsys, l, W0.S.lv[l].nu, B.nt[l], k, false, active, false, s);
    vm_mgb_launch_tail(B.dev, nsys, tail, active, s);
    if (tail == 0)
        vm_mgb_launch_dot_rz(B.dev, nsys, B.nb[0], k, active, B.ord, s);
    for (int l = tail - 1; l >= 0; --l)
        vm_mgb_launch_prolong(B.dev, nsys, l, W0.S.lv[l].nu, B.nt[l], k, active, B.ord && l == 0, s);
    vm_mgb_launch_dirspmv(B.dev, nsys, B.nb[0], k, active, B.ord, s);
}

// The set-up of a batch: nsys systems of one size whose workspaces are carved and whose type maps are enqueued on the
// context's stream.  Descriptors up, scalars and ordered-mode storage cleared, the hierarchy (level 0, coarsening) and its
// block / tile lists built, their counts read back.
int mgb_setup(vm_ctx *c, std::vector<MgbWork> &W, int nsys, MgbBatch &B)
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
    const bool fused = B.fused = mgb_fused(W[0].tail, W[0].S.lv[0].nu, MgbSwitches::from_environment().fuse_min, nsys);
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

// The look at the systems due after `it` completed iterations (mgb_iter_head(it) has been enqueued: x, r, r.r are theirs):
// one read-back of the span that holds them, then what each one's stop rule asks for (MgbStop::observe) -- the copy that
// keeps or brings back its best iterate, its bit of `active` cleared
int mgb_look(vm_ctx *c, std::vector<MgbWork> &W, MgbBatch &B, std::vector<MgbStop> &stop, int it, float tol, int max_it, uint64_t &active)
{
    hipStream_t s = c->stream;
    const MgbOrdLayout &Y = B.Y;
    const MgbSpan due = mgb_due_span(stop, active, it);
    if (due.hi < due.lo) return VM_OK;
    const size_t n_due = (size_t)(due.hi - due.lo + 1), x_bytes = (size_t)W[0].S.lv[0].w * W[0].S.lv[0].h * sizeof(VmV3);
    if (B.ord)
        VM_HIP(hipMemcpy2DAsync(&B.ord_head[(size_t)due.lo * Y.head], Y.head, B.ord_dev + (size_t)due.lo * Y.bytes, Y.bytes, Y.head, n_due,
                                hipMemcpyDeviceToHost, s));
    else
        VM_HIP(hipMemcpyAsync(&B.sc_host[due.lo], B.sc_dev + due.lo, n_due * sizeof(VmMgbScalars), hipMemcpyDeviceToHost, s));
    VM_HIP(hipStreamSynchronize(s));
    for (int i = due.lo; i <= due.hi; ++i) {
        if (!((active >> i) & 1) || !stop[i].due(it)) continue;
        // it == 0: parity 1, where k_mgb_init left r.r
        const int par = (it - 1) & 1;
        const double worst = B.ord ? mgb_rel_ordered(&B.ord_head[(size_t)i * Y.head], Y, par) : mgb_rel(B.sc_host[i], par);
        const int verdict = stop[i].observe(it, worst, tol, max_it, W[i].Xbest != nullptr);
        if (verdict & MGB_BREAKDOWN)
            return vm_fail(VM_E_NUMERIC, it == 0 ? "multigrid PCG: the right-hand side is not finite" : "multigrid PCG broke down (NaN)");
        if (verdict & MGB_SAVE_BEST) VM_HIP(hipMemcpyAsync(W[i].Xbest, W[i].S.X, x_bytes, hipMemcpyDeviceToDevice, s));
        if (verdict & MGB_STOP) active &= ~(1ull << i);
        if (verdict & MGB_RESTORE_BEST) VM_HIP(hipMemcpyAsync(W[i].S.X, W[i].Xbest, x_bytes, hipMemcpyDeviceToDevice, s));
    }
    return VM_OK;
}

// The batched PCG proper: nsys systems of one size whose workspaces are carved, whose type maps, right-hand sides
// (lv[0].b) and initial guesses (X) are enqueued on the context's stream.  Leaves every system's solution in its X
// (the iterate it stopped at; the best one seen near the tolerance if the workspace was carved with room for it), its
// iteration count and relative residual in iters / rels.
int mgb_solve(vm_ctx *c, std::vector<MgbWork> &W, int nsys, float tol, int max_it, int *iters, double *rels)
{
    hipStream_t s = c->stream;
    MgbBatch B;
    if (int rc = mgb_setup(c, W, nsys, B)) return rc;
    if (B.nb[0] == 0) {                     // no unknown anywhere: nothing to extend
        for (int i = 0; i < nsys; ++i) { iters[i] = 0; rels[i] = 0; }
        return VM_OK;
    }
    uint64_t active = nsys == 64 ? ~0ull : ((1ull << nsys) - 1);
    vm_mgb_launch_init(B.dev, nsys, B.nb[0], active, B.ord, s);
    B.sc_host.resize(nsys);
    std::vector<MgbStop> stop(nsys);
    std::vector<std::pair<VmEvent, VmEvent>> prof_ev;
    std::vector<int> prof_sys;
    if (int rc = mgb_look(c, W, B, stop, 0, tol, max_it, active)) return rc;
    for (int it = 0; active; ++it) {
        const bool probe = c->mgb_prof && it > 0;       // vm_dbg_poisson_profile: events around the launch that carries the update
        if (probe) {
            prof_ev.emplace_back();
            if (int rc = prof_ev.back().first.create()) return rc;
            if (int rc = prof_ev.back().second.create()) return rc;
            VM_HIP(hipEventRecord(prof_ev.back().first.get(), s));
        }
        mgb_iter_head(B, nsys, it, active, s);
        if (probe) {
            VM_HIP(hipEventRecord(prof_ev.back().second.get(), s));
            prof_sys.push_back(__builtin_popcountll(active));
        }
        if (it > 0) {
            if (int rc = mgb_look(c, W, B, stop, it, tol, max_it, active)) return rc;
            if (!active) break;
        }
        mgb_iter_rest(B, nsys, W[0], it, active, s);
        VM_HIP(hipGetLastError());
    }
    for (int i = 0; i < nsys; ++i) {
        iters[i] = stop[i].best_it;
        rels[i] = stop[i].best;
    }
    if (!prof_ev.empty()) {
        VM_HIP(hipStreamSynchronize(s));
        for (size_t k = 0; k < prof_ev.size(); ++k) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, prof_ev[k].first.get(), prof_ev[k].second.get()) == hipSuccess) {
                c->mgb_prof_us += 1e3 * ms;
                c->mgb_prof_launches += 1;
                c->mgb_prof_fused += B.fused ? 1 : 0;
                c->mgb_prof_unknown_launches += prof_sys[k];        // active systems of that launch (x unknowns per system: the caller's)
            }
        }
    }
    return VM_OK;
}

// What the entry points that solve share.  `solve(its, rel)` enqueues a solve of n systems on the context's stream and leaves
// their iteration counts and residuals; it runs between the context's two events, whose distance goes to *elapsed_ms.
// iters / rel_res (n entries each, optional) get the systems' results; `worst` is the system with the largest residual,
// which the caller turns into VM_E_NUMERIC if it is above the tolerance.
struct MgbResult {
    std::vector<int> its;
    std::vector<double> rel;
    int worst = 0;
};

template <class Solve>
int mgb_timed(vm_ctx *c, int n, Solve &&solve, int *iters, float *rel_res, float *elapsed_ms, MgbResult &R)
{
    hipStream_t s = c->stream;
    R.its.assign(n, 0);
    R.rel.assign(n, 0.0);
    VM_HIP(hipEventRecord(c->ev0.get(), s));
    if (int rc = solve(R.its.data(), R.rel.data())) return rc;
    VM_HIP(hipGetLastError());
    VM_HIP(hipEventRecord(c->ev1.get(), s));
    VM_HIP(hipEventSynchronize(c->ev1.get()));
    float ms = 0;
    VM_HIP(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()));
    if (elapsed_ms) *elapsed_ms = ms;
    for (int i = 0; i < n; ++i) {
        if (iters) iters[i] = R.its[i];
        if (rel_res) rel_res[i] = (float)R.rel[i];
        if (R.rel[i] > R.rel[R.worst]) R.worst = i;
    }
    return VM_OK;
}

} // namespace

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
    MgbResult R;
    auto solve = [&](int *its, double *rel) { return poisson_solve_batch(c, &f, &side, 1, tol, max_it, its, rel); };
    if (int rc = mgb_timed(c, 1, solve, iters, rel_res, elapsed_ms, R)) return rc;
    if (R.rel[0] > tol)
        return vm_fail(VM_E_NUMERIC, "vm_poisson_extend: residual %.3g after %d iterations (tol %.3g)", R.rel[0], R.its[0], (double)tol);
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
    std::vector<vm_frame *> fr(2 * n);
    std::vector<int> sd(2 * n);
    for (int i = 0; i < n; ++i) { fr[2 * i] = fr[2 * i + 1] = frames[i]; sd[2 * i] = 1; sd[2 * i + 1] = 2; }
    MgbResult R;
    auto solve = [&](int *its, double *rel) { return poisson_solve_batch(c, fr.data(), sd.data(), 2 * n, tol, max_it, its, rel); };
    if (int rc = mgb_timed(c, 2 * n, solve, iters, rel_res, elapsed_ms, R)) return rc;
    const int at = R.worst;
    if (R.rel[at] > tol)
        return vm_fail(VM_E_NUMERIC, "vm_poisson_extend_frames: residual %.3g after %d iterations on side %d of frame %d (tol %.3g)",
                       R.rel[at], R.its[at], at % 2 + 1, at / 2, (double)tol);
    return VM_OK;
}

// ---------------------------------------------------------------------------
// The same extension for the frame's float layers (vm_layer_ext.hip): the geometric type map, the fill from the
// other side's tight layer, and per group of up to three channels the RGB path's system through the same batched solver.

namespace {

int layer_groups(int channels) { return (channels + 2) / 3; }

// One side's workspace (pws2[side - 1], as mgb_system carves it) with the layers' type map, and its canvas and valid plane
// at ext / valid: the tight layer pasted, every outside cell filled from the other side's tight layer.  All enqueued.
int layer_prepare(vm_frame *f, int side, float *ext, uint8_t *valid, MgbWork &W)
{
    hipStream_t s = f->ctx->stream;
    if (int rc = f->pws2[side - 1].reserve(mgb_bytes(f->cw, f->ch))) return rc;
    mgb_carve(W, f->cw, f->ch, f->pws2[side - 1].get());
    const float *tight[2] = {f->layers.get(), f->layers.get() + f->layer_off};
    vm_layer_ext_launch_canvas(ext, valid, tight[side - 1], f->layer_ch, f->w, f->h, f->ex, s);
    vm_layer_ext_launch_type(W.type, f->w, f->h, f->ex, s);
    // the other side is the original tight layer (PoissonExt.cpp:54-57), the sign the side's (:104-137)
    vm_layer_ext_launch_fill(ext, valid, W.type, tight[side == 1 ? 1 : 0], f->v.get(), f->layer_ch, f->w, f->h, f->rs, f->ex,
                             side == 1 ? 1 : -1, s);
    VM_HIP(hipGetLastError());
    return VM_OK;
}

// room for the frame's two canvases, their valid planes and the groups' words
int layer_ext_reserve(vm_frame *f)
{
    hipStream_t s = f->ctx->stream;
    const size_t cells = (size_t)f->cw * f->ch, one = cells * f->layer_ch;
    f->lext_off = vm_align256(one * 4) / 4;
    if (int rc = f->lext.reserve(f->lext_off + one, s)) return rc;
    if (int rc = f->lext_valid.reserve(2 * cells, s)) return rc;
    return f->lext_nz.reserve(4, s);
}

// Both sides of every channel group, group by group on the frame's two workspaces: a batch of two systems per group, less
// those whose right-hand side is all zeros -- the system is positive definite, their solution is zero, and the solver
// (whose residual is relative to the right-hand side) is not asked.  its / rels: side 1 then side 2 of each group.
int layer_solve(vm_frame *f, float tol, int max_it, int *its, double *rels)
{
    vm_ctx *c = f->ctx;
    hipStream_t s = c->stream;
    const int C = f->layer_ch, cw = f->cw, ch = f->ch;
    const size_t cells = (size_t)cw * ch;
    float *ext[2] = {f->lext.get(), f->lext.get() + f->lext_off};
    uint8_t *valid[2] = {f->lext_valid.get(), f->lext_valid.get() + cells};
    std::vector<MgbWork> W(2);
    for (int k = 0; k < 2; ++k)
        if (int rc = layer_prepare(f, k + 1, ext[k], valid[k], W[k])) return rc;
    const int ng = layer_groups(C);
    for (int g = 0; g < ng; ++g) {
        const int c0 = 3 * g, n = std::min(3, C - c0);
        int *nz_dev = f->lext_nz.get();
        VM_HIP(hipMemsetAsync(nz_dev, 0, 2 * sizeof(int), s));
        for (int k = 0; k < 2; ++k)
            vm_layer_ext_launch_setup(ext[k], valid[k], W[k].type, W[k].S.lv[0].b, W[k].S.X, nz_dev + k, cw, ch, C, c0, n, s);
        VM_HIP(hipGetLastError());
        int nz[2] = {0, 0};
        VM_HIP(hipMemcpyAsync(nz, nz_dev, sizeof(nz), hipMemcpyDeviceToHost, s));
        VM_HIP(hipStreamSynchronize(s));
        std::vector<MgbWork> live;
        int at[2], nlive = 0;
        for (int k = 0; k < 2; ++k) {
            its[2 * g + k] = 0;
            rels[2 * g + k] = 0;
            if (nz[k]) { live.push_back(W[k]); at[nlive++] = k; }
            else VM_HIP(hipMemsetAsync(W[k].S.X, 0, cells * sizeof(VmV3), s));
        }
        if (nlive) {
            int li[2];
            double lr[2];
            if (int rc = mgb_solve(c, live, nlive, tol, max_it, li, lr)) return rc;
            for (int j = 0; j < nlive; ++j) { its[2 * g + at[j]] = li[j]; rels[2 * g + at[j]] = lr[j]; }
        }
        for (int k = 0; k < 2; ++k)
            vm_layer_ext_launch_paste(ext[k], valid[k], W[k].type, W[k].S.X, cw, ch, C, c0, n, g == ng - 1, s);
        VM_HIP(hipGetLastError());
    }
    return VM_OK;
}

} // namespace

// The frame's layers extended past the image edge as its canvases are (PoissonExt.cpp:49-362): from then on every layer
// render call samples the (ch, cw, C) canvases.  iters / rel_res: two entries per channel group, side 1 then side 2.  A failed
// call leaves the frame with its tight layers.
extern "C" int vm_frame_extend_layers(vm_frame *f, float tol, int max_it, int *iters, float *rel_res, float *elapsed_ms)
{
    VM_ENTER_LOCKED(f);
    if (!f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", __func__);
    if (f->ex == 0) return vm_fail(VM_E_STATE, "%s: the frame has no extension (ex == 0)", __func__);
    if (!(tol > 0) || max_it < 1) return vm_fail(VM_E_INVALID, "%s: bad argument", __func__);
    vm_ctx *c = f->ctx;
    f->layer_ext = false;
    if (int rc = layer_ext_reserve(f)) return rc;
    const int n = 2 * layer_groups(f->layer_ch);
    MgbResult R;
    auto solve = [&](int *its, double *rel) { return layer_solve(f, tol, max_it, its, rel); };
    if (int rc = mgb_timed(c, n, solve, iters, rel_res, elapsed_ms, R)) return rc;
    const int at = R.worst;
    if (R.rel[at] > tol)
        return vm_fail(VM_E_NUMERIC, "%s: residual %.3g after %d iterations on side %d of channel group %d (tol %.3g)", __func__,
                       R.rel[at], R.its[at], at % 2 + 1, at / 2, (double)tol);
    f->layer_ext = true;
    return VM_OK;
}

extern "C" int vm_frame_download_layers_ext(vm_frame *f, int side, float *out, int pitch_floats)
{
    if (!out || (side != 1 && side != 2)) return vm_fail(VM_E_INVALID, "%s: bad argument", __func__);
    VM_ENTER(f);
    if (!f->layer_ext) return vm_fail(VM_E_STATE, "%s: the frame's layers are not extended (vm_frame_extend_layers)", __func__);
    hipStream_t s = f->ctx->stream;
    const size_t row = (size_t)f->cw * f->layer_ch * 4;
    if (int rc = vm_copy_pitched(__func__, hipMemcpyDeviceToHost, f->lext.get() + (side - 1) * f->lext_off, row, out, pitch_floats, 4, row,
                                 f->ch, s)) return rc;
    VM_HIP(hipStreamSynchronize(s));
    return VM_OK;
}

extern "C" int vm_frame_drop_layer_extension(vm_frame *f)
{
    VM_ENTER(f);
    f->layer_ext = false;
    return VM_OK;
}

// One side's canvas as the solve would find it -- filled, with its valid plane, type map and the right-hand side
// (ch, cw, C) of every channel group -- from buffers of the call's own: the frame's extension, if it holds one, is not
// touched (the workspace is the solver's scratch).
extern "C" int vm_dbg_layers_prepare(vm_frame *f, int side, float *filled, uint8_t *valid, uint8_t *type, float *rhs)
{
    if (side != 1 && side != 2) return vm_fail(VM_E_INVALID, "%s: side %d", __func__, side);
    VM_ENTER_LOCKED(f);
    if (!f->layer_ch) return vm_fail(VM_E_STATE, "%s: the frame holds no layers (vm_frame_upload_layers)", __func__);
    hipStream_t s = f->ctx->stream;
    const int C = f->layer_ch;
    const size_t cells = (size_t)f->cw * f->ch;
    VmDev<float> ext;
    VmDev<uint8_t> val;
    VmDev<int> nz;
    if (int rc = ext.reserve(cells * C)) return rc;
    if (int rc = val.reserve(cells)) return rc;
    if (int rc = nz.reserve(1)) return rc;
    MgbWork W;
    if (int rc = layer_prepare(f, side, ext.get(), val.get(), W)) return rc;
    if (filled) VM_HIP(hipMemcpyAsync(filled, ext.get(), cells * C * 4, hipMemcpyDeviceToHost, s));
    if (valid) VM_HIP(hipMemcpyAsync(valid, val.get(), cells, hipMemcpyDeviceToHost, s));
    if (type) VM_HIP(hipMemcpyAsync(type, W.type, cells, hipMemcpyDeviceToHost, s));
    std::vector<float> b3(rhs ? cells * 3 : 0);
    for (int g = 0; rhs && g < layer_groups(C); ++g) {
        const int c0 = 3 * g, n = std::min(3, C - c0);
        vm_layer_ext_launch_setup(ext.get(), val.get(), W.type, W.S.lv[0].b, W.S.X, nz.get(), f->cw, f->ch, C, c0, n, s);
        VM_HIP(hipGetLastError());
        VM_HIP(hipMemcpyAsync(b3.data(), W.S.lv[0].b, cells * sizeof(VmV3), hipMemcpyDeviceToHost, s));
        VM_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < cells; ++i)
            for (int k = 0; k < n; ++k) rhs[i * C + c0 + k] = b3[3 * i + k];
    }
    VM_HIP(hipStreamSynchronize(s));        // (the call's buffers are freed on return)
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
    mgb_iter_head(B, 1, 0, 1ull, s);
    mgb_iter_rest(B, 1, W[0], 0, 1ull, s);
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
    MgbResult R;
    auto solve = [&](int *its, double *rel) {
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
        rc = mgb_solve(c, W, 1, tol, max_it, its, rel);
        if (rc != VM_OK) return rc;
        VM_HIP(hipMemsetAsync(W[0].S.sc, 0, sizeof(VmMgbScalars), s));
        vm_qpath_launch_sum3(W[0].S.X, f->w, f->h, sums, ord_part, s);
        vm_qpath_launch_shift3(W[0].S.X, f->w, f->h, sums, f->u.get(), f->rs, s);
        f->u_zero = false;
        return (int)VM_OK;
    };
    if (int rc = mgb_timed(c, 1, solve, iters, rel_res, elapsed_ms, R)) return rc;
    if (R.rel[0] > tol)
        return vm_fail(VM_E_NUMERIC, "vm_frame_quadratic_path: residual %.3g after %d iterations (tol %.3g)", R.rel[0], R.its[0], (double)tol);
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
