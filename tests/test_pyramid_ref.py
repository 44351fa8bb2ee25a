"""The pyramid builder's chain at its edges, on the CPU: the oracle against outputs of the REFERENCE'S OWN
resampling library for thin, tiny and odd frames and for flows that are enlarged, reduced 3 : 1, saturated
or tie the axis order (tests/golden/pyramid_edges_ref.npz, flow_edges_ref.npz; inputs from seeds,
tests/pyramid_cases.py), and the numpy statement tests/pyramid_ref.py against the oracle (float32) and
against itself (float64 against float32), so that the yardstick of tests/test_gpu_pyramid_stages.py is
itself pinned.  CPU only."""
import os

import numpy as np
import pytest

import pyramid_cases as PC
import pyramid_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
LUMA_GOLD = np.load(os.path.join(HERE, "golden", "pyramid_edges_ref.npz"))
FLOW_GOLD = np.load(os.path.join(HERE, "golden", "flow_edges_ref.npz"))

# the bounds the oracle is held to today (test_pyramid_oracle.py, test_flow_scale_matches_the_reference_library):
# the same float operations in the same order, up to an ulp of powf between builds of libm
LUMA_TOL, FLOW_TOL = 2e-4, 5e-5
# float64 against float32, in unit roundoffs u of float32.  scale() alone: a sample passes through two inverse
# filters (one per axis, each of infinity-norm <= 1 / (4/6 - 2/6) = 3, so 9 together) and about 16 roundings
# on the way, on planes of magnitude 1.5.  Flows: 64 u of the 100 px range.  Lumas: next to a hard edge a
# dark sample (where the curve's slope is 12.92) is a sum of bright ones, so its error is 16 u of magnitude 1,
# not of its own, carried through that slope and the x 255.
U32 = 2.0 ** -24
SCALE_F64_TOL = 9 * 16 * U32 * 1.5
LUMA_F64_TOL, FLOW_F64_TOL = 16 * U32 * 12.92 * 255, 64 * U32 * 100

SCALES = [(75, 52, 38, 26), (97, 65, 49, 33), (200, 120, 67, 40), (5, 7, 4, 6), (34, 33, 33, 32), (7, 5, 4, 3),
          (4, 3, 2, 2), (2, 2, 1, 1), (257, 3, 129, 2), (80, 40, 40, 20), (90, 160, 45, 80)]
# an axis that does not shrink goes through the curves (powf)
ENLARGE = [(64, 40, 100, 70), (33, 33, 33, 33), (40, 64, 70, 100), (12, 9, 13, 10), (3, 2, 3, 2), (1, 1, 2, 3),
           (2, 1, 1, 1), (1, 1, 1, 1), (65, 30, 33, 30)]


@pytest.mark.parametrize("case", sorted(PC.LUMA_EDGES))
def test_oracle_pyramid_matches_reference_library_at_the_edges(oracle, case):
    w, h, nl, _ = PC.LUMA_EDGES[case]
    want = LUMA_GOLD[case]
    got = np.concatenate([l.ravel() for l in oracle.luma_pyramid(PC.edge_rgb(case), nl)])
    assert got.shape == want.shape
    d = np.abs(got - want)
    assert d.max() <= LUMA_TOL, d.max()
    assert (d == 0).mean() > 0.5
    assert np.ptp(want) > 100 or want.size < 4          # black and saturated regions are in the frame


@pytest.mark.parametrize("case", sorted(PC.FLOW_EDGES))
def test_oracle_flow_scale_matches_reference_library_at_the_edges(oracle, case):
    w, h, wo, ho, amp, _ = PC.FLOW_EDGES[case]
    want = FLOW_GOLD[case]
    got = oracle.flow_scale(PC.edge_flow(case), wo, ho)
    assert got.shape == want.shape == (ho, wo, 2)
    d = np.abs(got - want)
    assert d.max() <= FLOW_TOL, d.max()
    assert (d == 0).mean() > 0.3, (d == 0).mean()
    ratio = wo / w if wo < w or ho < h else 1.0
    assert np.abs(want[..., 0]).max() <= 50 * ratio + 1e-4
    if amp >= 50:                                         # the reference clamps: the plateau sits at 50 px x ratio
        assert (np.abs(np.abs(want[..., 0]) - 50 * ratio) < 1e-4).mean() > 0.05


@pytest.mark.parametrize("case", sorted(PC.LUMA_EDGES))
def test_statement_luma_pyramid(oracle, case):
    _, _, nl, _ = PC.LUMA_EDGES[case]
    rgb = PC.edge_rgb(case)
    orc = oracle.luma_pyramid(rgb, nl)
    f32, f64 = R.luma_pyramid(rgb, nl, np.float32), R.luma_pyramid(rgb, nl)
    for a, b, c in zip(orc, f32, f64):
        assert b.dtype == np.float32 and c.dtype == np.float64 and a.shape == b.shape == c.shape
        assert np.abs(a - b).max() <= LUMA_TOL, np.abs(a - b).max()
        assert np.abs(c - b).max() <= LUMA_F64_TOL, np.abs(c - b).max()
    want = np.concatenate([l.ravel() for l in f64])
    assert np.abs(want - LUMA_GOLD[case]).max() <= LUMA_F64_TOL


@pytest.mark.parametrize("case", sorted(PC.FLOW_EDGES))
def test_statement_flow_scale(oracle, case):
    _, _, wo, ho, _, _ = PC.FLOW_EDGES[case]
    fl = PC.edge_flow(case)
    a, b, c = oracle.flow_scale(fl, wo, ho), R.flow_scale(fl, wo, ho, np.float32), R.flow_scale(fl, wo, ho)
    assert b.dtype == np.float32 and c.dtype == np.float64
    assert np.abs(a - b).max() <= FLOW_TOL, np.abs(a - b).max()
    assert np.abs(c - b).max() <= FLOW_F64_TOL, np.abs(c - b).max()
    assert np.abs(c - FLOW_GOLD[case]).max() <= FLOW_F64_TOL


@pytest.mark.parametrize("w,h,wo,ho", SCALES)
def test_statement_reductions_equal_the_oracle_bit_for_bit(oracle, w, h, wo, ho):
    """no powf on this path: numpy's float32 operations in the oracle's order give the oracle's bits"""
    p = PC.noise_planes(w, h, w * 1000 + h)
    a, b, c = oracle.scale_planes(p, wo, ho), R.scale(p, wo, ho, np.float32), R.scale(p, wo, ho)
    assert a.shape == b.shape == (3, ho, wo)
    assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), np.abs(a - b).max()
    assert np.abs(c - b).max() <= SCALE_F64_TOL, np.abs(c - b).max()      # planes span about -0.35 .. 1.5
    assert w * h < 100 or (p.min() < 0 and p.max() > 1)


@pytest.mark.parametrize("w,h,wo,ho", ENLARGE)
def test_statement_enlargements(oracle, w, h, wo, ho):
    p = PC.noise_planes(w, h, w * 1000 + h)
    a, b, c = oracle.scale_planes(p, wo, ho), R.scale(p, wo, ho, np.float32), R.scale(p, wo, ho)
    # the curve's slope is 12.92 on the linear segment and the uncurve's 2.4 * 1.5^1.4 at the top of the planes
    assert np.abs(a - b).max() <= SCALE_F64_TOL, np.abs(a - b).max()
    assert np.abs(c - b).max() <= SCALE_F64_TOL * 12.92, np.abs(c - b).max()


def test_axis_order_rule():
    assert R.columns_first(200, 120, 67, 40) and not R.columns_first(120, 200, 40, 67)
    assert not R.columns_first(80, 40, 40, 20)           # the tie: rows first
    # the two axes commute as real-valued operators, not as float32 ones: the order shows in the last bits only,
    # so only a bit-for-bit comparison can tell which one ran
    p = PC.noise_planes(200, 120, 5)
    rows_first = R.scale_axis(R.scale_axis(p, 67, 0, np.float32), 40, 1, np.float32)
    rule = R.scale(p, 67, 40, np.float32)
    assert not np.array_equal(rows_first, rule) and np.abs(rows_first - rule).max() <= SCALE_F64_TOL


def test_flow_concat_statement(oracle):
    rng = np.random.RandomState(3)
    f = (rng.randn(20, 30, 2) * 12).astype(np.float32)      # leaves the 30 x 20 frame on every side
    f[3:6, 4:9] = np.float32([2.0, -3.0])                   # whole-number displacements: floor == ceil
    g = rng.randn(20, 30, 2).astype(np.float32)
    a, b, c = oracle.flow_concat(f, g), R.flow_concat(f, g, np.float32), R.flow_concat(f, g)
    assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    assert np.abs(c - b).max() <= 16 * U32 * 64
    y, x = np.mgrid[0:20, 0:30]
    assert ((x + f[..., 0] < 0).any() and (x + f[..., 0] > 29).any() and (y + f[..., 1] < 0).any()
            and (y + f[..., 1] > 19).any())
    assert np.array_equal(c[3, 4], f[3, 4].astype(np.float64) + g[0, 6])


@pytest.mark.parametrize("w,h,wo,ho", SCALES + ENLARGE)
def test_a_constant_image_stays_constant(oracle, w, h, wo, ho):
    for v in (0.0, 0.002, 0.25, 1.0, 1.3, -0.1):
        p = np.full((3, h, w), v, dtype=np.float32)
        # a reduction keeps it to double rounding; the curves' exponents f32(1 / 2.4) and f32(2.4) are not
        # inverse to each other: x ** (1 + d) with |d| <= 2 u
        tol = 1e-12 if wo < w and ho < h else 4 * U32 * max(abs(v), 1.0)
        assert np.abs(R.scale(p, wo, ho) - np.float64(np.float32(v))).max() <= tol
        assert np.abs(oracle.scale_planes(p, wo, ho) - np.float32(v)).max() <= 64 * U32 * max(abs(v), 0.05)


@pytest.mark.parametrize("w,h,wo,ho", [(40, 28, 20, 14), (33, 21, 17, 11), (30, 20, 30, 20), (24, 16, 40, 30), (60, 36, 20, 12)])
def test_a_flow_beyond_the_range_comes_back_saturated(oracle, w, h, wo, ho):
    for amp in (50.0, 60.0, 500.0):
        fl = np.broadcast_to(np.float32([amp, -amp]), (h, w, 2)).copy()
        shrinks = wo < w or ho < h
        want = np.float64([50.0 * (np.float32(wo) / np.float32(w) if shrinks else 1), -50.0 * (np.float32(ho) / np.float32(h) if shrinks else 1)])
        for got in (oracle.flow_scale(fl, wo, ho), R.flow_scale(fl, wo, ho, np.float32), R.flow_scale(fl, wo, ho)):
            assert np.abs(got - want).max() <= FLOW_F64_TOL, (amp, np.abs(got - want).max())
