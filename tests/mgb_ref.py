"""Plain numpy statement of the compositor's linear solver (videomorphing_amd/csrc/vm_mgb.h, its host rules
vm_mgb_plan.h): the hierarchy, one V cycle
z = M^-1 r stage by stage, and the preconditioned CG around it.  Written from the header's description, not from the kernels'
structure: whole-grid arrays, one half-sweep at a time, nothing tiled, nothing fused, nothing "in differences".

Every function takes a `dtype`.  float64 is the reference the device is compared with; float32 is the SAME statement in the
device's precision and only sizes tolerances (tolerance()).  No GPU and no oracle are needed.

Conventions: arrays are (h, w) or (h, w, channels); we[y, x] is the weight of the edge (x, y) - (x + 1, y), shape
h x (w - 1); ws[y, x] of (x, y) - (x, y + 1), shape (h - 1) x w.
"""
import numpy as np

# vm_mgb_plan.h
COARSEST = 64            # VM_MGB_COARSEST: the hierarchy ends at a grid of at most this many cells ...
MAXLEV = 14              # VM_MGB_MAXLEV: ... or at this many levels
COARSE_SWEEPS = 2        # VM_MGB_COARSE_SWEEPS: symmetric sweeps each way on the coarsest grid
TAIL_X, TAIL_B, TAIL_PAIRS = 5120, 2048, 3072      # VM_MGB_TAIL_X / _B / _PAIRS
NU_POISSON, NU_QPATH = (1, 1, 2), (1,)             # VM_MGB_NU_POISSON / _QPATH


# ---------------------------------------------------------------------------
# the rules of the hierarchy (vm_mgb_plan.h: mg_sizes, mg_tail_level, mg_nu, mg_parse_nu), restated; tests/test_mgb_plan.py
# compares the two without a device

def sizes(w, h):
    """(w, h) per level: halved, rounding up, until <= COARSEST cells or MAXLEV levels"""
    v = [(w, h)]
    while v[-1][0] * v[-1][1] > COARSEST and len(v) < MAXLEV:
        v.append(((v[-1][0] + 1) // 2, (v[-1][1] + 1) // 2))
    return v


def tail_level(sz):
    """the first level of the one-workgroup tail (mg_tail_level): going up from the coarsest level, a level joins the
    tail while the tail's levels and the one above fit TAIL_X cells, the tail's levels fit TAIL_B, and the level above
    holds at most TAIL_PAIRS pairs of cells, ceil(w / 2) h"""
    below, l = 0, len(sz) - 1
    while l > 0:
        here, up = sz[l][0] * sz[l][1], sz[l - 1][0] * sz[l - 1][1]
        if below + here + up > TAIL_X or below + here > TAIL_B or (sz[l - 1][0] + 1) // 2 * sz[l - 1][1] > TAIL_PAIRS:
            break
        below += here
        l -= 1
    return l


def nu_levels(sz, table=NU_POISSON):
    """sweeps each way per level (mg_nu): table[l], the last entry repeats, cut to 2 on the levels above the tail"""
    tail = tail_level(sz)
    out = []
    for l in range(len(sz)):
        n = table[min(l, len(table) - 1)]
        out.append(n if l >= tail else min(n, 2))
    return out


def parse_nu(text):
    """VM_MGB_NU's syntax: every digit 1 .. 9 is an entry"""
    return tuple(int(ch) for ch in text if ch in "123456789")


# ---------------------------------------------------------------------------
# the operator of a level

class Level:
    """(A u)(p) = dg(p) u(p) - sum over p's edges of w u(neighbour); dg = screening + incident weights; dg == 0: p is not
    an unknown"""

    def __init__(self, we, ws, sc, dtype=np.float64):
        self.dtype = dtype
        self.h, self.w = sc.shape
        self.we, self.ws = we.astype(dtype), ws.astype(dtype)
        self.sc = np.maximum(sc, 0).astype(dtype)
        dg = self.sc.copy()
        dg[:, :-1] += self.we
        dg[:, 1:] += self.we
        dg[:-1] += self.ws
        dg[1:] += self.ws
        self.dg = dg
        self.unk = dg > 0
        self.inv = np.where(self.unk, dtype(1) / np.where(self.unk, dg, dtype(1)), dtype(0)).astype(dtype)
        yy, xx = np.mgrid[0:self.h, 0:self.w]
        self.red = ((xx + yy) & 1) == 0

    def nbsum(self, x):
        s = np.zeros_like(x)
        s[:, :-1] += self.we[..., None] * x[:, 1:]
        s[:, 1:] += self.we[..., None] * x[:, :-1]
        s[:-1] += self.ws[..., None] * x[1:]
        s[1:] += self.ws[..., None] * x[:-1]
        return s

    def apply(self, x):
        return self.dg[..., None] * x - self.nbsum(x)

    def half(self, x, b, red):
        """one Gauss-Seidel half-sweep over the unknowns of one colour, in place"""
        m = (self.red == red) & self.unk
        x[m] = (self.inv[..., None] * (b + self.nbsum(x)))[m]

    def full_we(self):
        """we / ws as the device stores them: h x w, the missing last column / row zero"""
        a = np.zeros((self.h, self.w), self.dtype)
        a[:, :-1] = self.we
        return a

    def full_ws(self):
        a = np.zeros((self.h, self.w), self.dtype)
        a[:-1] = self.ws
        return a

    def coarsen(self):
        """2x2 aggregation, piecewise-constant transfer: a coarse edge = half the sum of the fine edges that cross the
        aggregates' common boundary; the screening is summed"""
        h2, w2 = (self.h + 1) // 2, (self.w + 1) // 2

        def pad(a):
            out = np.zeros((2 * h2, 2 * w2), self.dtype)
            out[:a.shape[0], :a.shape[1]] = a
            return out
        wef, wsf, scf = pad(self.we), pad(self.ws), pad(self.sc)
        half = self.dtype(0.5)
        we = (half * (wef[0::2, 1::2] + wef[1::2, 1::2]))[:, :w2 - 1]      # fine edges at odd x leave to the east
        ws = (half * (wsf[1::2, 0::2] + wsf[1::2, 1::2]))[:h2 - 1]         # ... at odd y to the south
        sc = scf[0::2, 0::2] + scf[0::2, 1::2] + scf[1::2, 0::2] + scf[1::2, 1::2]
        return Level(we, ws, sc, self.dtype)


def level0(unknown, tie, dtype=np.float64):
    """level 0 from a mask of unknowns and a screening term: unit weights between neighbouring unknowns"""
    unknown = np.asarray(unknown, bool)
    E = (unknown[:, :-1] & unknown[:, 1:]).astype(dtype)
    S = (unknown[:-1] & unknown[1:]).astype(dtype)
    return Level(E, S, np.where(unknown, tie, 0).astype(dtype), dtype)


def level0_of_types(typ, dtype=np.float64):
    """... from the Poisson extension's type map: unknown <=> type > 0, ring pixels (type 1) tied to their colour"""
    return level0(typ > 0, (typ == 1), dtype)


def hierarchy(L0):
    levels = [L0]
    for _ in sizes(L0.w, L0.h)[1:]:
        levels.append(levels[-1].coarsen())
    return levels


# ---------------------------------------------------------------------------
# the cycle

def restrict(r):
    h, w = r.shape[:2]
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    p = np.zeros((2 * h2, 2 * w2, r.shape[2]), r.dtype)
    p[:h, :w] = r
    return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]


def prolong(xc, h, w):
    return np.repeat(np.repeat(xc, 2, axis=0), 2, axis=1)[:h, :w]


def cycle(levels, r, nu):
    """z = M^-1 r.  nu: sweeps each way per level (nu_levels).  Returns (z, b, x): b[l] the right-hand side and x[l] the
    result of level l's cycle (b[0] = r on the unknowns, x[0] = z)"""
    n = len(levels)
    b, x = [None] * n, [None] * n
    dt = levels[0].dtype
    b[0] = np.where(levels[0].unk[..., None], r, 0).astype(dt)
    for l in range(n - 1):                       # down: red, black from zero; residual; restriction
        L = levels[l]
        x[l] = np.zeros_like(b[l])
        for _ in range(nu[l]):
            L.half(x[l], b[l], True)
            L.half(x[l], b[l], False)
        res = b[l] - L.apply(x[l])
        res[~L.unk] = 0
        b[l + 1] = restrict(res)
        b[l + 1][~levels[l + 1].unk] = 0
    L = levels[-1]                               # the coarsest grid: symmetric sweeps from zero
    x[-1] = np.zeros_like(b[-1])
    for _ in range(COARSE_SWEEPS):
        L.half(x[-1], b[-1], True)
        L.half(x[-1], b[-1], False)
    for _ in range(COARSE_SWEEPS):
        L.half(x[-1], b[-1], False)
        L.half(x[-1], b[-1], True)
    for l in range(n - 2, -1, -1):               # up: correction; black, red
        L = levels[l]
        x[l] += prolong(x[l + 1], L.h, L.w)
        x[l][~L.unk] = 0
        for _ in range(nu[l]):
            L.half(x[l], b[l], False)
            L.half(x[l], b[l], True)
    return x[0], b, x


def half_steps(levels, r, nu):
    """the cycle again with every level's sweeps written as repeated applications of ONE-sweep half-steps on a fresh copy
    (no state kept between sweeps but the iterate): what a kernel that makes two sweeps at once must equal"""
    def one_sweep(L, x, b, first_red):
        y = x.copy()
        L.half(y, b, first_red)
        L.half(y, b, not first_red)
        return y
    dt = levels[0].dtype

    def rec(l, b):
        L = levels[l]
        x = np.zeros_like(b)
        if l == len(levels) - 1:
            for _ in range(COARSE_SWEEPS):
                x = one_sweep(L, x, b, True)
            for _ in range(COARSE_SWEEPS):
                x = one_sweep(L, x, b, False)
            return x
        for _ in range(nu[l]):
            x = one_sweep(L, x, b, True)
        res = b - L.apply(x)
        res[~L.unk] = 0
        bc = restrict(res)
        bc[~levels[l + 1].unk] = 0
        x = x + prolong(rec(l + 1, bc), L.h, L.w)
        x[~L.unk] = 0
        for _ in range(nu[l]):
            x = one_sweep(L, x, b, False)
        return x
    return rec(0, np.where(levels[0].unk[..., None], r, 0).astype(dt))


# ---------------------------------------------------------------------------
# the PCG

def pcg(levels, B, X0, nu, tol, max_it=60):
    """the device's iteration: x from X0, r = B - A x, z = M^-1 r, p = z + beta p, q = A p, alpha = r.z / p.q per channel;
    stops at the first iteration count N whose worst channel of sqrt(r.r / b.b) is <= tol (the device looks at the
    residual at the cadence of vm_mgb_plan.h: MgbStop and can stop up to three iterations later).  Dot products are float64
    sums of `dtype` vectors, alpha and beta are rounded to `dtype`, as on the device.  Returns (N or -1, [rel after 0, 1,
    ... iterations], x)"""
    L = levels[0]
    dt = L.dtype
    m = L.unk[..., None]
    B = np.where(m, B, 0).astype(dt)
    x = np.where(m, X0, 0).astype(dt)
    r = np.where(m, B - L.apply(x), 0).astype(dt)

    def dot(a, c):
        return (a.astype(np.float64) * c.astype(np.float64)).sum(axis=(0, 1))
    bb = dot(B, B)
    safe = np.where(bb > 0, bb, 1)
    hist = []
    p = rz_old = None
    for it in range(max_it + 1):
        rr = dot(r, r)
        hist.append(float(np.sqrt(np.where(bb > 0, rr / safe, 0).max())))
        if hist[-1] <= tol:
            return it, hist, x
        if it == max_it:
            break
        z = cycle(levels, r, nu)[0]
        rz = dot(r, z)
        if p is None:
            p = z
        else:
            p = z + np.where(rz_old > 0, rz / np.where(rz_old > 0, rz_old, 1), 0).astype(dt) * p
        rz_old = rz
        q = L.apply(p)
        pq = dot(p, q)
        al = np.where(pq > 0, rz / np.where(pq > 0, pq, 1), 0).astype(dt)
        x = x + al * p
        r = r - al * q
    return -1, hist, x


def poisson_system(ext, typ):
    """right-hand side and initial guess of the Poisson extension (vm_poisson.hip: k_setup) from a PREPARED canvas (classified,
    outside pixels filled) and its type map, float64: b = colour of a ring pixel + the gradients of the filled colours
    across the edges between unknowns; x0 = the colour that stands there, mid grey on unfilled (marker) pixels"""
    col = ext[..., :3].astype(np.float64)
    marker = (ext[..., 0] == 255) & (ext[..., 1] == 0) & (ext[..., 2] == 255) & (ext[..., 3] == 0)
    t2 = (typ > 1) & ~marker
    gx, gy = np.zeros(col.shape), np.zeros(col.shape)
    ok = t2[:, 1:] & t2[:, :-1]
    gx[:, 1:][ok] = (col[:, 1:] - col[:, :-1])[ok]
    ok = t2[1:] & t2[:-1]
    gy[1:][ok] = (col[1:] - col[:-1])[ok]
    unk = typ > 0
    E = unk[:, :-1] & unk[:, 1:]
    S = unk[:-1] & unk[1:]
    B = np.zeros(col.shape)
    B[typ == 1] += col[typ == 1]
    B[1:][S] += gy[1:][S]
    B[:, 1:][E] += gx[:, 1:][E]
    B[:, :-1][E] -= gx[:, 1:][E]
    B[:-1][S] -= gy[1:][S]
    B[~unk] = 0
    X0 = np.where(marker[..., None], 128.0, col)
    X0[~unk] = 0
    return B, X0


def classify(ext):
    """the type map of a canvas (PoissonExt.cpp:59-101): 2 = outside (alpha > 0), 1 = an inside pixel next to one, 0 = the rest"""
    out = ext[..., 3] > 0
    nb = np.zeros_like(out)
    nb[1:] |= out[:-1]
    nb[:-1] |= out[1:]
    nb[:, 1:] |= out[:, :-1]
    nb[:, :-1] |= out[:, 1:]
    return np.where(out, 2, np.where(nb, 1, 0)).astype(np.int32)


# ---------------------------------------------------------------------------
# tolerances: nothing is sized from the device's output

def tolerance(ref64, ref32):
    """the bound for a device quantity on one level, relative to the quantity's max norm there: 8 x the deviation of the
    statement's float32 run from its float64 run (accumulation order inside a tile differs from numpy's, FMA contraction
    is legal), at least 16 float32 ulps.  Returns (absolute bound, the float32 run's relative deviation)"""
    scale = float(np.abs(ref64).max())
    dev32 = float(np.abs(ref32.astype(np.float64) - ref64).max()) / scale if scale > 0 else 0.0
    rel = max(8.0 * dev32, 16.0 * float(np.finfo(np.float32).eps))
    return rel * scale, dev32
