"""Cases and helpers of the FAST audits (tests/test_gpu_fast_audit.py) -- oracle only, importable without a GPU.

The audits hold VM_MATH_FAST to the CPU oracle where the rest of the suite compares FAST with FAST: under point
constraints that PULL (the constraint term does work: the footprint pixels move 0.55 - 1.33 px in one sweep), under the
boundary conditions, on ragged and sub-tile levels.  Everything a bound is built from is computed here from the oracle
alone; tests/test_fast_audit_cases.py asserts, on the CPU, that the oracle itself stays inside every cap on these cases.

Pixel classes (every bound is asserted per class, so a fault in a few pixels cannot hide in an allowance sized for a level):
  footprint  oracle ui_axy > 0 (the texels a constraint is splatted on: 17 - 18 pixels)
  ring       within 2 of the image border, not footprint
  rest       everything else
"""
import collections
import functools

import numpy as np

import oracle as O
from videomorphing_amd import synth

BCOND_NONE, BCOND_CORNER, BCOND_BORDER = 0, 1, 2
PULL = 1.5                                        # px a constraint's target lies from v0
CLASSES = ("footprint", "ring", "rest")
INCREMENTAL = ("luma", "mean", "var", "cross", "value", "tps_b", "ui_b")     # what a sweep maintains
UNTOUCHED = ("counter", "tps_axy", "ui_axy")                                   # what it must not write
ALT = dict(w_ui=1e3, eps=0.003, ssim_clamp=0.3)                                # the second parameter set

Case = collections.namedtuple("Case", "name w h bcond constrained seed params")


def _case(w, h, bcond, constrained=True, seed=0, params=()):
    tag = {BCOND_NONE: "none", BCOND_CORNER: "corner", BCOND_BORDER: "border"}[bcond]
    name = "%dx%d-%s%s%s" % (w, h, tag, "" if constrained else "-free", "-alt" if params else "")
    return Case(name, w, h, bcond, constrained, seed, tuple(sorted(dict(params).items())))


# 33x12: with seed 0 one interior pixel lands 0.040 px apart under two commit orders of the ORACLE (a line search on the
# edge between two brackets), and with seed 1 the fold-over test pins one footprint pixel; SEED_33x12 is the first seed at
# which the oracle's four orders stay within eps in every class and every footprint pixel moves (spread 0.0017 / 0.0048 /
# 0.0052 px, moves >= 0.87 px; tests/test_fast_audit_cases.py asserts both)
SEED_33x12 = 2

SWEEP_CASES = [
    _case(150, 97, BCOND_BORDER),                 # several tiles, ragged in both directions
    _case(69, 21, BCOND_CORNER),                  # exactly one tile pitch
    _case(120, 68, BCOND_NONE),
    _case(333, 47, BCOND_BORDER),                 # five tiles wide
    _case(33, 12, BCOND_BORDER, seed=SEED_33x12),  # smaller than a tile, every pixel within 6 of a border
    _case(12, 11, BCOND_BORDER, constrained=False),   # all 25 border classes and little else
    _case(120, 68, BCOND_NONE, params=ALT),
]
STATE_CASES = [c for c in SWEEP_CASES if c.constrained]
FIXED_POINT_CASES = [_case(120, 68, BCOND_BORDER), _case(96, 64, BCOND_NONE)]
FIXED_POINT_CAP = 2000
STATE_SWEEPS = (1, 20)


def by_name(name):
    for c in SWEEP_CASES + FIXED_POINT_CASES:
        if c.name == name:
            return c
    raise KeyError(name)


def params(case):
    return O.default_params(bcond=case.bcond, **dict(case.params))


def points(w, h):
    """halfway points of the constraints: two interior ones at fractional positions (four-texel footprints), one in
    each of two opposite border classes, one next to the row BCOND_BORDER locks; the first twice (duplicates add up)"""
    p = [(0.3 * w + 0.4, 0.4 * h + 0.3), (0.7 * w + 0.5, 0.6 * h + 0.5), (1.5, 1.5), (w - 2.5, h - 2.5), (0.5 * w, 1.0)]
    return p + p[:1]


def start_field(case):
    rng = np.random.RandomState(case.seed)
    return (0.8 * synth.displacement(case.w, case.h) + 0.05 * rng.randn(case.h, case.w, 2)).astype(np.float32)


def constraints(case, v0=None):
    """constraint k: halfway point (x, y), target t = v0[y, x] + PULL (cos 2.4 k, sin 2.4 k) -- (x - t, y - t, x + t,
    y + t, weight 1) in the coordinates of the level itself (w0, h0 = w, h)"""
    if not case.constrained:
        return np.zeros((0, 5), np.float32)
    v0 = start_field(case) if v0 is None else v0
    out = []
    for k, (x, y) in enumerate(points(case.w, case.h)):
        t = v0[int(y), int(x)].astype(np.float64) + PULL * np.array([np.cos(2.4 * k), np.sin(2.4 * k)])
        out.append((x - t[0], y - t[1], x + t[0], y + t[1], 1.0))
    return np.asarray(out, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def start(case):
    """(img0, img1, v0, constraints) of a case; shared, never written to"""
    i0, i1 = synth.make_pair(case.w, case.h)
    v0 = start_field(case)
    cons = constraints(case, v0)
    for a in (i0, i1, v0, cons):
        a.setflags(write=False)
    return i0, i1, v0, cons


def oracle_level(case, v=None):
    """a fresh oracle level of the case holding field v (default: the start), init + splat done, full mask"""
    i0, i1, v0, cons = start(case)
    lo = O.Level(case.w, case.h)
    lo.set_images(i0, i1)
    lo.field("v")[...] = v0 if v is None else v
    lo.init(params(case).ssim_clamp)
    lo.splat(case.w, case.h, cons)
    return lo


def snapshot(lvl, fields=INCREMENTAL + UNTOUCHED):
    return {f: np.array(lvl.field(f), copy=True) for f in fields}


@functools.lru_cache(maxsize=None)
def class_masks(case):
    """{class: (h, w) bool}; the footprint is where the ORACLE's splat put weight"""
    w, h = case.w, case.h
    lo = oracle_level(case)                       # field() is a view: the level must outlive its use
    foot = lo.field("ui_axy") > 0
    y, x = np.mgrid[0:h, 0:w]
    near = (x < 2) | (y < 2) | (x >= w - 2) | (y >= h - 2)
    return {"footprint": foot, "ring": near & ~foot, "rest": ~near & ~foot}


def locked_mask(case):
    """the pixels the boundary condition never lets move (pixel_on_border of the reference, BCOND_CORNER's right-hand
    corners never matching, as it is written there)"""
    w, h = case.w, case.h
    m = np.zeros((h, w), bool)
    if case.bcond == BCOND_BORDER:
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    elif case.bcond == BCOND_CORNER:
        m[0, 0] = m[-1, 0] = True
    return m


def class_max(d, masks):
    """{class: max of d over the class} (0 for an empty class)"""
    return {c: float(d[masks[c]].max()) if masks[c].any() else 0.0 for c in CLASSES}


class commit_order(object):
    """with commit_order(k): the oracle folds a phase's commits in order k (0 row-major ... 3), 0 again afterwards"""

    def __init__(self, order):
        self.order = order

    def __enter__(self):
        O.lib().vmo_set_commit_order(self.order)

    def __exit__(self, *a):
        O.lib().vmo_set_commit_order(0)


@functools.lru_cache(maxsize=None)
def oracle_sweeps(case, sweeps=1, order=0):
    """the oracle's v after `sweeps` sweeps from the start under commit order `order` (read-only)"""
    lo = oracle_level(case)
    P = params(case)
    with commit_order(order):
        for _ in range(sweeps):
            lo.optimize_iter(P)
    v = np.array(lo.field("v"), copy=True)
    v.setflags(write=False)
    return v


def pixel_diff(a, b):
    """|dv| per pixel as test_fast_mode_tolerance measures it after one sweep: the larger component"""
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(-1)


def oracle_order_spread(case):
    """{class: largest |dv| between any two of the oracle's four commit orders after one sweep}"""
    masks = class_masks(case)
    vs = [oracle_sweeps(case, 1, k) for k in range(4)]
    out = dict.fromkeys(CLASSES, 0.0)
    for a in range(4):
        for b in range(a + 1, 4):
            m = class_max(pixel_diff(vs[a], vs[b]), masks)
            out = {c: max(out[c], m[c]) for c in CLASSES}
    return out


def state_error(state, case, v):
    """{field: max |state[field] - the field a fresh init + splat builds from v|} and the fresh fields' magnitudes"""
    fresh = snapshot(oracle_level(case, v))
    err = {f: float(np.abs(state[f].astype(np.float64) - fresh[f]).max()) for f in fresh}
    mag = {f: float(np.abs(fresh[f]).max()) for f in fresh}
    return err, mag, fresh


@functools.lru_cache(maxsize=None)
def oracle_drift(case, sweeps):
    """D_f of Audit 2: the oracle's own incremental arrays after `sweeps` sweeps against a fresh init + splat from its own
    v.  Returns (D, magnitude, largest |ui_b| change between start and end)."""
    lo = oracle_level(case)
    ui0 = np.array(lo.field("ui_b"), copy=True)
    P = params(case)
    for _ in range(sweeps):
        lo.optimize_iter(P)
    err, mag, _ = state_error(snapshot(lo), case, np.array(lo.field("v"), copy=True))
    return err, mag, float(np.abs(lo.field("ui_b") - ui0).max())


def state_tolerance(case, sweeps):
    """{field: max(8 D_f, 4 float32 ulps of the field's largest magnitude)}: eight is generous to fused multiply-adds
    and another summation tree; a dropped or mis-weighted update is wrong by the step times a coefficient, decades above"""
    D, mag, _ = oracle_drift(case, sweeps)
    return {f: max(8.0 * D[f], 4.0 * float(np.spacing(np.float32(mag[f])))) for f in INCREMENTAL}


def fresh_sweep(case, v):
    """hand v to a fresh oracle level (init, splat, full mask), one sweep: ({class: largest move}, commits, energy() of v)"""
    lo = oracle_level(case, v)
    P = params(case)
    energy = lo.energy(P)
    stats = np.zeros(4, np.float64)
    lo.optimize_iter(P, stats)
    move = pixel_diff(lo.field("v"), v)
    return class_max(move, class_masks(case)), int(stats[2]), energy


@functools.lru_cache(maxsize=None)
def oracle_fixed_point(case, order):
    """the oracle run to convergence from the start under commit order `order`:
    (v, sweeps, {class: largest move of a fresh sweep from v}, commits of that sweep, energy() of v)"""
    lo = oracle_level(case)
    with commit_order(order):
        iters = lo.optimize(params(case), FIXED_POINT_CAP)
    v = np.array(lo.field("v"), copy=True)
    v.setflags(write=False)
    move, commits, energy = fresh_sweep(case, v)
    return v, iters, move, commits, energy


def fixed_point_yardstick(case):
    """the reference's own figures over commit orders 0 - 2: (largest move of a fresh sweep from a fixed point, relative
    spread of the constraint totals, largest RMS distance between two fixed points)"""
    runs = [oracle_fixed_point(case, k) for k in range(3)]
    figure = max(max(r[2].values()) for r in runs)
    eu = [r[4][2] for r in runs]
    spread = (max(eu) - min(eu)) / eu[0] if eu[0] else 0.0
    rms = max(rms_distance(runs[a][0], runs[b][0]) for a in range(3) for b in range(a + 1, 3))
    return figure, spread, rms


def rms_distance(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).sum(-1).mean()))


# ---- the conditions that give the bounds teeth: asserted on the oracle alone, by the CPU test and again by each audit ----

# one sweep: |dv| <= EPS on >= 99 % of a class and <= 2 EPS on all of it (footprint: every pixel <= 2 EPS) -- the figures of
# test_gpu_parity.test_fast_mode_tolerance, in pixels.  They are NOT scaled with a case's own eps: the oracle's scatter
# between its commit orders comes from the window sums' rounding moving a bracket of the line search, not from the line
# search's resolution -- at eps = 0.003 (ALT) it measures 0.0015 / 0.0069 / 0.0055 px, at eps = 0.01 0.0011 / 0.0053 /
# 0.0083 px on the same level.
EPS = 0.01
MIN_MOVE = 0.5                                    # px every free footprint pixel moves in the oracle's sweep
MIN_EFFECT = 4 * EPS                              # ALT (w_ui 100 x weaker): what the constraints change at every footprint pixel


def check_sweep_conditions(case):
    """Audit 1's preconditions; returns the figures {"move": (min, max), "spread": {class: px}}"""
    masks, lock = class_masks(case), locked_mask(case)
    v0, v1 = start(case)[2], oracle_sweeps(case, 1, 0)
    move = pixel_diff(v1, v0)
    out = {"move": None, "spread": oracle_order_spread(case)}
    if case.constrained:
        n = int(masks["footprint"].sum())
        assert 17 <= n <= 18, (case.name, n)
        free = masks["footprint"] & ~lock
        if case.params:
            # a hundred times weaker constraints pull less than MIN_MOVE; what matters is that a sweep WITHOUT the term
            # lands at least twice the cap of 2 EPS away, at every footprint pixel
            effect = pixel_diff(v1, oracle_sweeps(case._replace(constrained=False, name=case.name + "-free"), 1, 0))
            out["effect"] = (float(effect[free].min()), float(effect[free].max()))
            assert effect[free].min() >= MIN_EFFECT, (case.name, out["effect"])
        else:
            assert move[free].min() >= MIN_MOVE, (case.name, float(move[free].min()))
        out["move"] = (float(move[free].min()), float(move[free].max()))
    else:
        assert not masks["footprint"].any()
    if case.bcond == BCOND_BORDER:
        assert lock.sum() == 2 * (case.w + case.h) - 4 and not move[lock].any(), case.name
    elif case.bcond == BCOND_CORNER:
        # the two left corners are locked; the right ones are free, as the reference writes the test -- and do move
        assert not move[lock].any() and move[0, -1] > 0 and move[-1, -1] > 0, case.name
    assert move[~lock].max() > 0.05, case.name
    for c in CLASSES:
        assert out["spread"][c] <= EPS, (case.name, c, out["spread"])
    return out


def check_state_conditions(case, sweeps):
    """Audit 2's preconditions: the yardsticks are non-zero and finite, the untouched arrays untouched, ui_b exercised"""
    D, mag, ui_change = oracle_drift(case, sweeps)
    for f in INCREMENTAL:
        assert 0 < D[f] < np.inf and 0 < mag[f] < np.inf, (case.name, sweeps, f, D[f], mag[f])
    for f in UNTOUCHED:
        assert D[f] == 0, (case.name, sweeps, f)
    assert ui_change > 0.1, (case.name, sweeps, ui_change)
    return D, mag, ui_change


def check_fixed_point_conditions(case):
    """Audit 3's preconditions: the oracle converges under orders 0 - 2 and a fresh sweep from each of its fixed points
    commits only rounding-level moves, all below EPS; returns fixed_point_yardstick(case)"""
    for k in range(3):
        v, iters, move, commits, energy = oracle_fixed_point(case, k)
        assert iters < FIXED_POINT_CAP, (case.name, k, iters)
        assert commits > 0 and max(move.values()) < EPS, (case.name, k, commits, move)
        assert energy[2] > 0, (case.name, k, energy)
    figure, spread, rms = fixed_point_yardstick(case)
    assert rms <= 0.02, (case.name, rms)           # the RMS bound FAST gets must hold among the oracle's own fixed points
    return figure, spread, rms
