"""What test_gpu_mgb_stages.py, its child processes and test_mgb_ref.py share: the test canvases, the access to the
device's hierarchy and cycle through vm_dbg_mgb_*, and the stage-by-stage comparison with tests/mgb_ref.py.  No test here."""
import ctypes as C

import numpy as np

import mgb_ref
from videomorphing_amd import capi, morph, synth

QPATH = capi.DBG_MGB_QPATH


# ---------------------------------------------------------------------------
# inputs

def canvas_case(cw, ch, ex, seed):
    """two extended canvases of cw x ch with a margin of ex, holes punched into both the way
    test_poisson_on_random_outside_regions does (rectangles and single pixels of alpha 255: unknowns inside otherwise empty
    tiles, blocks with one unknown, coarse cells without any), and a halfway field"""
    w, h = cw - 2 * ex, ch - 2 * ex
    rng = np.random.RandomState(seed)
    rgb0, rgb1 = synth.make_rgb_pair(w, h, frame=seed)
    v = (0.6 * synth.displacement(w, h) + 0.2 * rng.randn(h, w, 2)).astype(np.float32)
    e0, e1 = morph.make_extended(rgb0, ex).copy(), morph.make_extended(rgb1, ex).copy()
    for e in (e0, e1):
        for _ in range(6):
            rw, rh = rng.randint(1, min(24, w) + 1), rng.randint(1, min(12, h) + 1)
            x0, y0 = rng.randint(0, w - rw + 1), rng.randint(0, h - rh + 1)
            if rw * rh * 8 <= w * h:                     # (a thin canvas keeps most of its inside)
                e[ex + y0:ex + y0 + rh, ex + x0:ex + x0 + rw, 3] = 255
        for _ in range(10):
            e[ex + rng.randint(0, h), ex + rng.randint(0, w), 3] = 255
    return e0, e1, v


def residual(unk, seed, channels=3):
    """a seeded random field on the unknowns, float32 (what both the device and the statement get)"""
    r = np.random.RandomState(seed).randn(unk.shape[0], unk.shape[1], 3).astype(np.float32)
    r[..., channels:] = 0
    r[~unk] = 0
    return r


# ---------------------------------------------------------------------------
# the device, through the hooks

def dev_setup(fr, which):
    L = fr._L
    nlev, tail = C.c_int(0), C.c_int(0)
    arr = [(C.c_int * mgb_ref.MAXLEV)() for _ in range(5)]
    capi.check(L.vm_dbg_mgb_setup(fr._h, which, C.byref(nlev), C.byref(tail), *arr))
    n = nlev.value
    w, h, nu, nb, nt = ([int(a[l]) for l in range(n)] for a in arr)
    return dict(nlev=n, tail=tail.value, sizes=list(zip(w, h)), nu=nu, nblocks=nb, ntiles=nt)


def dev_level(fr, which, l, w, h):
    dg, we, ws = (np.zeros((h, w), np.float32) for _ in range(3))
    b, x = (np.full((h, w, 3), np.nan, np.float32) for _ in range(2))
    have = C.c_int(0)
    capi.check(fr._L.vm_dbg_mgb_level(fr._h, which, l, dg.ctypes.data, we.ctypes.data, ws.ctypes.data, b.ctypes.data,
                                      x.ctypes.data, C.byref(have)))
    return dict(dg=dg, we=we, ws=ws, b=b if have.value & 1 else None, x=x if have.value & 2 else None)


def dev_cycle(fr, which, r):
    r = np.ascontiguousarray(r, np.float32)
    z, q = np.zeros_like(r), np.zeros_like(r)
    capi.check(fr._L.vm_dbg_mgb_cycle(fr._h, which, r.ctypes.data, z.ctypes.data, q.ctypes.data))
    return z, q


# ---------------------------------------------------------------------------
# the statement of a system, both precisions

class Statement:
    def __init__(self, unknown, tie, table):
        self.lv = {dt: mgb_ref.hierarchy(mgb_ref.level0(unknown, tie, dt)) for dt in (np.float64, np.float32)}
        self.sizes = mgb_ref.sizes(unknown.shape[1], unknown.shape[0])
        self.tail = mgb_ref.tail_level(self.sizes)
        self.nu = mgb_ref.nu_levels(self.sizes, table)
        self.unk = self.lv[np.float64][0].unk

    def cycle(self, r):
        """{dtype: (z, b, x, q)} of one cycle on the float32 field r"""
        out = {}
        for dt, lv in self.lv.items():
            z, b, x = mgb_ref.cycle(lv, r.astype(dt), self.nu)
            out[dt] = (z, b, x, lv[0].apply(z))
        return out


def statement_of_canvas(ext, table):
    typ = mgb_ref.classify(ext)
    return Statement(typ > 0, typ == 1, table)


def statement_of_grid(w, h, table):
    return Statement(np.ones((h, w), bool), np.zeros((h, w)), table)


# ---------------------------------------------------------------------------
# comparisons.  Each returns a list of report lines "shape stage level: float32 model deviation, device deviation"; a
# mismatch raises with the first level and stage that is off and the worst cell.

def _worst(d):
    y, x = np.unravel_index(int(np.argmax(d.max(axis=-1) if d.ndim == 3 else d)), d.shape[:2])
    return int(x), int(y)


def compare(name, stage, l, dev, ref64, ref32, mask, report):
    """the device's `dev` against the statement on the cells of `mask`, with the tolerance rule of mgb_ref.tolerance"""
    m = mask if ref64.ndim == 2 else mask[..., None]
    r64, r32 = np.where(m, ref64, 0), np.where(m, ref32, 0)
    bound, dev32 = mgb_ref.tolerance(r64, r32)
    d = np.abs(np.where(m, dev.astype(np.float64), 0) - r64)
    d = np.where(np.isfinite(d), d, np.inf)
    scale = float(np.abs(r64).max())
    worst = float(d.max())
    report.append("%s %s level %d: float32 model %.2e, device %.2e (bound %.2e, relative to %.3g)" % (
        name, stage, l, dev32, worst / scale if scale > 0 else worst, bound / scale if scale > 0 else bound, scale))
    print(report[-1])
    assert worst <= bound, "%s: %s of level %d is off: |device - float64| = %.3g at (x, y) = %s, bound %.3g (float32 model: %.3g relative)" % (
        name, stage, l, worst, _worst(d), bound, dev32)


def check_hierarchy(name, fr, which, S, report):
    """a: nlev, tail, sizes, nu equal the restated rules; dg, we, ws of every level equal the statement's -- exactly where its
    float32 run is exact (level 0 always: small integers), else within the tolerance rule"""
    info = dev_setup(fr, which)
    assert info["nlev"] == len(S.sizes) and info["sizes"] == S.sizes, (name, info["sizes"], S.sizes)
    assert info["tail"] == S.tail, (name, info["tail"], S.tail)
    assert info["nu"] == S.nu, (name, info["nu"], S.nu)
    for l, (w, h) in enumerate(S.sizes):
        D = dev_level(fr, which, l, w, h)
        L64, L32 = S.lv[np.float64][l], S.lv[np.float32][l]
        everywhere = np.ones((h, w), bool)
        for stage, dev, r64, r32 in (("dg", D["dg"], L64.dg, L32.dg), ("we", D["we"], L64.full_we(), L32.full_we()),
                                     ("ws", D["ws"], L64.full_ws(), L32.full_ws())):
            if l == 0 or np.array_equal(r32.astype(np.float64), r64):
                d = np.abs(dev.astype(np.float64) - r64)
                assert d.max() == 0, "%s: %s of level %d is off (exact values): %.3g at (x, y) = %s" % (name, stage, l, d.max(), _worst(d))
            else:
                compare(name, stage, l, dev, r64, r32, everywhere, report)
        # the lists the kernels sweep hold every block / tile with an unknown
        gx, gy = (w + 63) // 64, (h + 3) // 4
        pad = np.zeros((16 * ((gy + 3) // 4), gx * 64), bool)
        pad[:h, :w] = L64.unk
        assert info["nblocks"][l] == int(pad.reshape(-1, 4, gx, 64).any(axis=(1, 3)).sum()), (name, l)
        assert info["ntiles"][l] == int(pad.reshape(-1, 16, gx, 64).any(axis=(1, 3)).sum()), (name, l)
    return info


def check_cycle(name, fr, which, S, r, report):
    """b: one cycle on the device against the float64 cycle on the same operator and r: b[l + 1] of every level above the
    tail, x[l] of every level down to the tail, z, q = A z.  Returns the device's (z, q)."""
    z, q = dev_cycle(fr, which, r)
    ref = S.cycle(r)
    (z64, b64, x64, q64), (z32, b32, x32, q32) = ref[np.float64], ref[np.float32]
    for l in range(S.tail):
        w, h = S.sizes[l + 1]
        D = dev_level(fr, which, l + 1, w, h)
        assert D["b"] is not None, (name, l + 1)
        compare(name, "b (pre-smoothing, residual, restriction of level %d)" % l, l + 1, D["b"], b64[l + 1], b32[l + 1],
                S.lv[np.float64][l + 1].unk, report)
    for l in range(S.tail, -1, -1):
        w, h = S.sizes[l]
        D = dev_level(fr, which, l, w, h)
        assert D["x"] is not None, (name, l)
        stage = "x (the tail)" if l == S.tail else "x (prolongation, post-smoothing)"
        compare(name, stage, l, D["x"], x64[l], x32[l], S.lv[np.float64][l].unk, report)
    for l in range(S.tail + 1, len(S.sizes)):
        D = dev_level(fr, which, l, *S.sizes[l])
        assert D["b"] is None and D["x"] is None, (name, l)
    compare(name, "z", 0, z, z64, z32, S.unk, report)
    compare(name, "q = A z", 0, q, q64, q32, S.unk, report)
    return z, q


def check_symmetry(name, fr, which, S, pairs, report):
    """c: <u, M v> == <M u, v> and <u, M u> > 0 from the device's outputs, in float64.  The bound: the tolerance rule applied
    to the inner product -- the float32 statement's own deviation of <u, M v> from the float64 one, times 8, relative to
    |u| |M v| (at least 16 ulps of it)"""
    for k, (u, v) in enumerate(pairs):
        Mu, Mv = dev_cycle(fr, which, u)[0].astype(np.float64), dev_cycle(fr, which, v)[0].astype(np.float64)
        u64, v64 = u.astype(np.float64), v.astype(np.float64)
        a, b = float((u64 * Mv).sum()), float((Mu * v64).sum())
        m64 = mgb_ref.cycle(S.lv[np.float64], v64, S.nu)[0]
        m32 = mgb_ref.cycle(S.lv[np.float32], v.astype(np.float32), S.nu)[0].astype(np.float64)
        scale = float(np.sqrt((u64 * u64).sum() * (m64 * m64).sum()))
        dev32 = abs(float((u64 * m32).sum()) - float((u64 * m64).sum())) / scale
        bound = max(8 * dev32, 16 * float(np.finfo(np.float32).eps)) * scale
        report.append("%s symmetry pair %d: float32 model %.2e, device |<u,Mv> - <Mu,v>| %.2e (bound %.2e, relative to |u||Mv| = %.3g)" % (
            name, k, dev32, abs(a - b) / scale, bound / scale, scale))
        print(report[-1])
        assert abs(a - b) <= bound, "%s: M is not symmetric on the device: <u, M v> = %.9g, <M u, v> = %.9g, bound %.3g (pair %d)" % (name, a, b, bound, k)
        uMu = float((u64 * Mu).sum())
        assert uMu > 0, "%s: <u, M u> = %.3g (pair %d)" % (name, uMu, k)


def corner_field(S, seed):
    """a field supported on the unknowns among the corner cells of ONE 64 x 16 tile (the 2 x 2 cells in each of its corners)"""
    h, w = S.unk.shape
    rng = np.random.RandomState(seed)
    best = None
    for ty in range((h + 15) // 16):
        for tx in range((w + 63) // 64):
            m = np.zeros((h, w), bool)
            x0, y0, x1, y1 = 64 * tx, 16 * ty, min(64 * tx + 64, w), min(16 * ty + 16, h)
            for ys in (slice(y0, y0 + 2), slice(max(y1 - 2, y0), y1)):
                for xs in (slice(x0, x0 + 2), slice(max(x1 - 2, x0), x1)):
                    m[ys, xs] = True
            m &= S.unk
            if best is None or m.sum() > best.sum():
                best = m
    r = rng.randn(h, w, 3).astype(np.float32)
    r[~best] = 0
    assert best.sum() > 0
    return r


# ---------------------------------------------------------------------------
# the systems by name

def open_case(ctx, cw, ch, ex, seed):
    e0, e1, v = canvas_case(cw, ch, ex, seed)
    fr = morph.Frame(ctx, cw - 2 * ex, ch - 2 * ex, ex)
    fr.upload(e0, e1, v, None)
    return fr, e0, e1, v


def poisson_table():
    import os
    env = mgb_ref.parse_nu(os.environ.get("VM_MGB_NU", ""))
    return env or mgb_ref.NU_POISSON


def qpath_table():
    import os
    env = mgb_ref.parse_nu(os.environ.get("VM_MGB_NU", ""))
    return env or mgb_ref.NU_QPATH


CYCLE_SHAPES = [(380, 260, 40), (65, 17, 3), (129, 33, 3), (26, 18, 4), (3, 1700, 1)]
SYMMETRY_SHAPES = [(380, 260, 40), (65, 17, 3)]


def run_cycle_shapes(ctx, report, shapes=CYCLE_SHAPES, qpath=True):
    """b (and the hierarchy on the way) on every shape, both sides' canvases alternating; the quadratic path once at 160 x 110"""
    for k, (cw, ch, ex) in enumerate(shapes):
        fr, e0, e1, _ = open_case(ctx, cw, ch, ex, 31 + k)
        try:
            side = 1 + k % 2
            S = statement_of_canvas((e0, e1)[side - 1], poisson_table())
            name = "%dx%d side %d" % (cw, ch, side)
            check_hierarchy(name, fr, side, S, report)
            check_cycle(name, fr, side, S, residual(S.unk, 100 + k), report)
        finally:
            fr.close()
    if qpath:
        fr, _, _, _ = open_case(ctx, 160 + 2, 110 + 2, 1, 40)
        try:
            S = statement_of_grid(160, 110, qpath_table())
            check_hierarchy("160x110 qpath", fr, QPATH, S, report)
            check_cycle("160x110 qpath", fr, QPATH, S, residual(S.unk, 140, channels=2), report)
        finally:
            fr.close()


def run_symmetry_shapes(ctx, report, shapes=SYMMETRY_SHAPES):
    for k, (cw, ch, ex) in enumerate(shapes):
        fr, e0, _, _ = open_case(ctx, cw, ch, ex, 51 + k)
        try:
            S = statement_of_canvas(e0, poisson_table())
            pairs = [(residual(S.unk, 200 + 2 * j), residual(S.unk, 201 + 2 * j)) for j in range(4)]
            pairs.append((corner_field(S, 300), residual(S.unk, 301)))
            pairs.append((corner_field(S, 302), corner_field(S, 303)))
            check_symmetry("%dx%d side 1" % (cw, ch), fr, 1, S, pairs, report)
        finally:
            fr.close()


def child_main():
    """what a child process of test_gpu_mgb_stages.py runs under its own VM_MGB_NU: b and c on all their shapes"""
    ctx = morph.Context(0)
    report = []
    run_cycle_shapes(ctx, report)
    run_symmetry_shapes(ctx, report)
    ctx.close()
    print("MGB_STAGES_OK", len(report))


# ---------------------------------------------------------------------------
# f: iteration counts.  The inputs are chosen on the CPU so that the float64 history is not near a crossing of the
# tolerance (safe_count); the table is re-derived by test_mgb_ref.py.

TOLS = (1e-4, 1e-5)


def poisson_reference(oracle, cw, ch, ex, seed, side, dtype, tol=min(TOLS)):
    """the statement's PCG on the system the device solves for that side: (history, the canvases and v)"""
    e0, e1, v = canvas_case(cw, ch, ex, seed)
    w, h = cw - 2 * ex, ch - 2 * ex
    ext, other = (e0, e1) if side == 1 else (e1, e0)
    filled, typ, _ = oracle.poisson_prepare(ext, w, h, ex, other[ex:ex + h, ex:ex + w].copy(), v, side)
    B, X0 = mgb_ref.poisson_system(filled, typ)
    lv = mgb_ref.hierarchy(mgb_ref.level0_of_types(typ, dtype))
    nu = mgb_ref.nu_levels(mgb_ref.sizes(cw, ch), mgb_ref.NU_POISSON)
    return mgb_ref.pcg(lv, B, X0, nu, tol)[1]


def qpath_rhs(jo):
    """the quadratic path's right-hand side (QuadraticPath.cpp:137-170) from the per-pixel optimal Jacobians, zero mean"""
    h, w = jo.shape[:2]
    j = jo.astype(np.float64)
    B = np.zeros((h, w, 3))
    B[1:, :, 0] += j[1:, :, 1]
    B[1:, :, 1] += j[1:, :, 3] - 1
    B[:, 1:, 0] += j[:, 1:, 0] - 1
    B[:, 1:, 1] += j[:, 1:, 2]
    B[:, :-1, 0] -= j[:, 1:, 0] - 1
    B[:, :-1, 1] -= j[:, 1:, 2]
    B[:-1, :, 0] -= j[1:, :, 1]
    B[:-1, :, 1] -= j[1:, :, 3] - 1
    return B - B.mean(axis=(0, 1))


def qpath_field(w, h, seed, noise):
    """a smooth halfway field plus `noise` hundredths of a pixel of white noise"""
    rng = np.random.RandomState(seed)
    return (0.5 * synth.displacement(w, h) + 0.01 * noise * rng.randn(h, w, 2)).astype(np.float32)


def qpath_reference(oracle, w, h, noise, seed, dtype, tol=1e-4):
    jo = oracle.quadratic_path(qpath_field(w, h, seed, noise), tol=1e-3, max_it=10, want_jopt=True)[3]
    S = mgb_ref.hierarchy(mgb_ref.level0(np.ones((h, w), bool), np.zeros((h, w)), dtype))
    nu = mgb_ref.nu_levels(mgb_ref.sizes(w, h), mgb_ref.NU_QPATH)
    B = qpath_rhs(jo)
    return mgb_ref.pcg(S, B, np.zeros_like(B), nu, tol)[1]


def safe_count(h64, h32, tol):
    """N of the float64 history if it is a safe expectation -- rel[N] <= tol / 2, rel[N - 1] >= 2 tol, and the float32 run
    of the statement stops at the same N -- else None"""
    n64 = next((i for i, r in enumerate(h64) if r <= tol), None)
    n32 = next((i for i, r in enumerate(h32) if r <= tol), None)
    if n64 is None or n64 == 0 or n32 != n64:
        return None
    return n64 if h64[n64] <= tol / 2 and h64[n64 - 1] >= 2 * tol else None


# (kind, w, h, ex, seed, side, tol, N): canvases w x h with a margin of ex for "poisson"; a frame of w x h whose field carries ex
# hundredths of a pixel of noise for "qpath".  Chosen by trying seeds 60, 61, ... (sides 1, 2) in turn until safe_count accepted
# one -- and, where twenty seeds gave none (380 x 260 at 1e-4 with a margin of 40 sits at 0.9 tol after five iterations whatever
# the seed; the quadratic path with 5 hundredths at 1.1 .. 1.9 tol after four), another margin / noise level.  N is the float64
# statement's count.
ITERATION_TABLE = [
    ("poisson", 160, 110, 10, 62, 1, 1e-4, 5),
    ("poisson", 160, 110, 10, 64, 1, 1e-5, 6),
    ("poisson", 333, 47, 10, 60, 2, 1e-4, 5),
    ("poisson", 333, 47, 10, 61, 1, 1e-5, 6),
    ("poisson", 380, 260, 50, 60, 1, 1e-4, 5),
    ("poisson", 380, 260, 40, 66, 1, 1e-5, 7),
    ("qpath", 160, 110, 2, 60, 0, 1e-4, 5),
]
