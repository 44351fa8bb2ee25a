"""The wave-wide line search samples its known points four at a time, one per octet of each half of the wave (the ladder,
profiles/line_search_ladder.md), and gives the bits it gave when every round sampled its own point.

1  Sampling only.  vm_dbg_ladder runs the search text the sweep kernels expand on the energy f(t) = t, under which the
   search walks its whole ladder from cc down to eps, on two 9x7 images, a wave per case in one launch.  Per point it
   returns the lumas the ladder delivered and the lumas of the one-point taps32 the generic loop still runs -- the code
   tests/test_gpu_line_search_round.py and its fixtures hold to the parent.  All bits equal; the points are the float32
   ladder of the search (multiply, multiply, add; then one multiply per point), stated here in numpy; the lumas of
   the finite cases are a bilinear, clamped sample of the images (float64 statement, within 1e-3 of 0 .. 255 values:
   the positions are reproduced to the bit but for double rounding, the weights' products carry a few float32 ulps
   of 255).
2  Sweeps.  tests/golden/line_search_ladder.json was recorded by tests/golden/make_line_search_ladder.py with the
   library of the PARENT commit, never with the code under test: SHA-256 of v after 40 sweeps at 75x26 in FAST
   arithmetic and the activity counters of every sweep, under forced PASS / STEP / SPLIT, once with the temporal term
   in every round's energy and once with pulling point constraints and the locks of BCOND_BORDER
   (tests/line_search_ladder_cases.py)."""
import json
import os

import numpy as np
import pytest

import line_search_cases as LC
import line_search_ladder_cases as LL
from videomorphing_amd import capi

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_search_ladder.json")))

# ---- 1: the sampling ---------------------------------------------------------------------------------------------------

W, H = 9, 7
EPS = np.float32(2.0 ** -9)               # cc = 10 then takes 9 rounds: a third batch
POINTS, WORDS = 40, 201
R = np.float32(0.618033989)
C1 = np.float32(1.0) - R


def ladder_points(cc, eps):
    """the points the search evaluates under f(t) = t, in order: the initial pair, then two per round while cc > eps"""
    cc = np.float32(cc)
    b = cc * C1
    x = b * R + cc * C1
    pts = [b, x]
    while cc > eps:                       # fx < fb never holds: f grows with t
        xn = b * R
        xn2 = xn * R
        pts += [xn, xn2]
        if not x > eps:                   # the guess fails: one shift, cc <- x <= eps ends the search
            break
        cc, x, b = b, xn, xn2
    return pts


def ladder_cases():
    """(name, px, py, vx, vy, gx, gy, cc)"""
    eps = float(EPS)
    above = float(np.nextafter(EPS, np.float32(1)))
    s = float(np.sqrt(0.5))
    dirs = [(1, 0), (-1, 0), (0, 1), (0, -1), (s, s), (-s, s), (s, -s), (-s, -s), (0.6, 0.8), (-0.28, 0.96)]
    out = []
    for k, (gx, gy) in enumerate(dirs):                                     # interior
        for cc in (0.0, eps, above, 0.5, 3.0, 10.0):
            out.append(("interior", 4, 3, 0.3 - 0.05 * k, -0.2 + 0.07 * k, gx, gy, cc))
    border = [(0, 0), (8, 0), (0, 6), (8, 6), (4, 0), (4, 6), (0, 3), (8, 3)]
    for k, (px, py) in enumerate(border):                                   # edges and corners
        gx, gy = dirs[k % len(dirs)]
        ox, oy = (1.0 if px == 0 else -1.0 if px == 8 else 0.0), (1.0 if py == 0 else -1.0 if py == 6 else 0.0)
        for cc in (eps, 3.0, 10.0):
            out.append(("one_image", px, py, 1.6 * ox + 0.1, 1.3 * oy - 0.1, gx, gy, cc))      # p - v leaves, p + v stays
            out.append(("one_image", px, py, -1.6 * ox + 0.1, -1.3 * oy - 0.1, gx, gy, cc))    # the other image
            out.append(("both_images", px, py, 9.5 * (ox or 1.0), 7.25 * (oy or -1.0), gx, gy, cc))
            out.append(("outside", px, py, 100.0 * (ox or 1.0), -64.5 * (oy or 1.0), gx, gy, cc))
    for frac in (0.3, 0.66, 0.1, 0.9):                                      # a texel boundary between two octets' points
        for gx, gy in dirs[:6]:
            out.append(("straddle", 4, 3, gx * (frac - 1.0), gy * (frac - 1.0), gx, gy, 10.0))
            out.append(("straddle", 5, 2, -0.5 * frac, 0.5 * frac, gx, gy, 6.0))
    nan = float("nan")
    for vx, vy in ((nan, 0.5), (0.5, nan), (nan, nan)):                     # NaN in v
        for cc in (0.0, 3.0, 10.0):
            out.append(("nan", 4, 3, vx, vy, 0.6, 0.8, cc))
            out.append(("nan", 0, 6, vx, vy, -s, s, cc))
    return out


def images():
    rng = np.random.RandomState(97)
    return (rng.uniform(0.0, 255.0, (H, W)).astype(np.float32), rng.uniform(0.0, 255.0, (H, W)).astype(np.float32))


def bilinear(img, x, y):
    """tex2D(linear, clamp) at texel coordinates (x, y), float64"""
    fi, fj = np.floor(x), np.floor(y)
    a, b = x - fi, y - fj
    fi, fj = np.clip(fi, -1, W), np.clip(fj, -1, H)
    i0, i1 = int(np.clip(fi, 0, W - 1)), int(np.clip(fi + 1, 0, W - 1))
    j0, j1 = int(np.clip(fj, 0, H - 1)), int(np.clip(fj + 1, 0, H - 1))
    im = img.astype(np.float64)
    return (1 - a) * (1 - b) * im[j0, i0] + a * (1 - b) * im[j0, i1] + (1 - a) * b * im[j1, i0] + a * b * im[j1, i1]


@pytest.fixture(scope="module")
def ladder_run(gpu_ctx):
    cases = ladder_cases()
    i0, i1 = images()
    params = np.zeros((len(cases), 8), np.float32)
    for k, c in enumerate(cases):
        params[k, :7] = c[1:]
    got = np.zeros((len(cases), WORDS), np.uint32)
    capi.check(gpu_ctx._L.vm_dbg_ladder(gpu_ctx._h, W, H, i0.ctypes.data, i1.ctypes.data, len(cases), params.ctypes.data, float(EPS),
                                        got.ctypes.data))
    return cases, params, got


def test_ladder_cases_cover_the_batches(ladder_run):
    cases, params, got = ladder_run
    n = {k: len(ladder_points(c[7], EPS)) for k, c in enumerate(cases)}
    # rounds 0 .. 3 come from the first batch, 4 .. 7 from the second, 8 .. from the third: two points a round
    assert min(n.values()) == 2 and max(n.values()) >= 2 * 9 and max(n.values()) <= POINTS
    assert {"interior", "one_image", "both_images", "outside", "straddle", "nan"} == {c[0] for c in cases}
    for fam in ("one_image", "both_images", "outside", "straddle", "nan"):
        assert max(n[k] for k, c in enumerate(cases) if c[0] == fam) >= 2 * 9, fam
    # straddle: consecutive points of one half, four rounds apart at the most, fall into different texels
    for k, c in enumerate(cases):
        if c[0] == "straddle" and c[7] == 10.0:
            t = np.array(ladder_points(c[7], EPS)[:8:2], np.float64)
            cells = {(int(np.floor(4 - (c[3] + c[5] * u))), int(np.floor(3 - (c[4] + c[6] * u)))) for u in t}
            assert len(cells) > 1, c


def test_ladder_points_are_the_searchs(ladder_run):
    cases, params, got = ladder_run
    for k, c in enumerate(cases):
        want = np.array(ladder_points(c[7], EPS), np.float32).view(np.uint32)
        assert got[k, 0] == len(want), (c, got[k, 0], len(want))
        assert np.array_equal(got[k, 1:1 + 5 * len(want):5], want), c
        assert not got[k, 1 + 5 * len(want):].any(), c


def test_ladder_lumas_are_the_one_point_taps_bits(ladder_run):
    cases, params, got = ladder_run
    bad = []
    for k, c in enumerate(cases):
        rec = got[k, 1:1 + 5 * int(got[k, 0])].reshape(-1, 5)
        if not np.array_equal(rec[:, 1:3], rec[:, 3:5]):
            bad.append((c, np.argwhere(rec[:, 1:3] != rec[:, 3:5])[:4].tolist()))
    assert not bad, (len(bad), bad[:6])


def test_ladder_lumas_are_a_bilinear_sample(ladder_run):
    cases, params, got = ladder_run
    i0, i1 = images()
    worst = 0.0
    for k, c in enumerate(cases):
        rec = got[k, 1:1 + 5 * int(got[k, 0])].reshape(-1, 5)
        lum = rec[:, 1:3].copy().view(np.float32)
        if c[0] == "nan":
            assert np.isnan(lum).any(axis=1).all(), c                 # a NaN coordinate poisons that image's weights
            continue
        px, py, vx, vy, gx, gy = [np.float64(q) for q in params[k, :6]]
        for p, t in enumerate(rec[:, 0].copy().view(np.float32).astype(np.float64)):
            nvx, nvy = np.float64(np.float32(gx * t + vx)), np.float64(np.float32(gy * t + vy))
            x0, y0 = np.float64(np.float32(px - nvx)), np.float64(np.float32(py - nvy))
            x1, y1 = np.float64(np.float32(px + nvx)), np.float64(np.float32(py + nvy))
            e = max(abs(lum[p, 0] - bilinear(i0, x0, y0)), abs(lum[p, 1] - bilinear(i1, x1, y1)))
            worst = max(worst, e)
            assert e <= 1e-3, (c, p, t, lum[p], bilinear(i0, x0, y0), bilinear(i1, x1, y1))
    print("ladder lumas against the float64 bilinear sample: worst %.3g" % worst)


# ---- 2: the sweeps -----------------------------------------------------------------------------------------------------

_got = {}


def _case(ctx, family, name, sched, parts):
    """each case is run once and shared"""
    if (family, name) not in _got:
        _got[(family, name)] = LL.run_case(ctx, family, name, sched, parts)
    return _got[(family, name)]


@pytest.fixture(scope="module")
def fast_ctx(gpu_ctx):
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    yield gpu_ctx
    gpu_ctx.set_math_mode(capi.MATH_EXACT)


def test_fixture_covers_the_cases():
    assert GOLDEN["sweeps"] == LL.SWEEPS and GOLDEN["counters"] == list(LC.COUNTERS) and "parent commit" in GOLDEN["library"]
    assert GOLDEN["size"] == [LL.W, LL.H]
    assert sorted(GOLDEN["cases"]) == sorted(LL.key(f, n) for f, n, _, _ in LL.cases())
    # every forced schedule ran its own kernels when the fixtures were made, moved pixels, and kept searching to the end
    for k, c in GOLDEN["cases"].items():
        per = GOLDEN["per_sweep_tables"][c["per_sweep_table"]]
        assert c["reached"], k
        assert all(i == LL.SWEEPS for i in c["iters"]) and len(per) == LL.SWEEPS, k
        assert all(t[2] > 0 for t in c["totals"]) and all(p[1] > 0 for p in per[-1]), k
        if "/temporal/" in k:
            assert c["temp_mask_max"] > 0 and len(c["totals"]) == 2, k       # the term was there, on both pages


@pytest.mark.parametrize("family,name,sched,parts", LL.cases())
def test_schedule_reproduces_the_parent_bits(fast_ctx, family, name, sched, parts):
    want = GOLDEN["cases"][LL.key(family, name)]
    got = _case(fast_ctx, family, name, sched, parts)
    print(LL.key(family, name), got["v_sha256"][:16], got["totals"], got["sched_launches"])
    assert got["sched_launches"][LC.SLOT[name]] > 0          # the kernels the case is about ran
    assert got["iters"] == want["iters"]
    assert got["per_sweep"] == GOLDEN["per_sweep_tables"][want["per_sweep_table"]]
    assert got["totals"] == want["totals"]
    assert got["v_sha256"] == want["v_sha256"]
    assert got["v_sha256_single_sweeps"] == want["v_sha256_single_sweeps"]
    if family == "temporal":
        assert got["temp_mask_max"] == want["temp_mask_max"] > 0


@pytest.mark.parametrize("family", LL.FAMILIES)
def test_schedules_still_equal_each_other(fast_ctx, family):
    """PASS == STEP == SPLIT bit for bit, in the parent and now"""
    got = {n: _case(fast_ctx, family, n, s, p)["v_sha256"] for n, s, p in LL.SCHEDULES}
    gold = {n: GOLDEN["cases"][LL.key(family, n)]["v_sha256"] for n, _, _ in LL.SCHEDULES}
    assert len(set(gold.values())) == 1 and len(set(got.values())) == 1, (family, gold, got)
