"""The numpy statement of the error view (tests/error_ref.py) against the CPU oracle's vmo_energy, and
known answers of its sampling and ramp.  No GPU."""
import numpy as np

import error_ref as R
from videomorphing_amd import capi, synth


def test_statement_totals_agree_with_the_oracle_energy(oracle):
    """after init and three sweeps at 138x84 with three constraints the float32 planes add up to Level.energy(P)
    within 8 2^-24 sum|e| + n 2^-53 sum|e| per term: at most six float32 roundings per plane value against vmo_energy's
    float64 expression of the same arrays, plus the textbook summation bound -- computed from the planes themselves"""
    w, h = 138, 84
    P = oracle.default_params(bcond=capi.BCOND_BORDER)
    i0, i1 = synth.make_pair(w, h)
    lo = oracle.Level(w, h)
    lo.set_images(i0, i1)
    lo.field("v")[...] = (0.8 * synth.displacement(w, h)).astype(np.float32)
    lo.init(P.ssim_clamp)
    lo.splat(w, h, R.constraints(w, h))
    for _ in range(3):
        lo.optimize_iter(P)
    assert (lo.field("ui_axy") > 0).any()
    e = R.planes(lo.field("value"), lo.field("v"), lo.field("tps_b"), lo.field("ui_axy"), lo.field("ui_b"),
                 np.float32(1.0) / np.float32(w * h), P)
    assert e.dtype == np.float32 and e.shape == (5, h, w)
    assert not e[R.TEMP].any()
    assert np.array_equal(e[R.ALL], (e[R.SSIM] + e[R.TPS]) + e[R.UI])
    want = lo.energy(P)
    got = R.totals(e)
    for k in (R.SSIM, R.TPS, R.UI):
        print("term %d: statement %.17g oracle %.17g bound %.3g" % (k, got[k], want[k], R.statement_bound(e[k])))
        assert abs(got[k] - want[k]) <= R.statement_bound(e[k]), k
        assert got[k] != 0
    # e_all adds two float32 roundings per pixel to the three terms' own (at most six of the eight the factor covers)
    assert abs(R.exact_totals(e)[R.ALL] - want.sum()) <= sum(R.statement_bound(e[k]) for k in range(3))


def test_temporal_term_and_flag():
    P = capi.KernParams(w_temp=10.0, w_ui=1e5, w_tps=0.05, w_ssim=100.0)
    h, w = 3, 4
    z1, z2 = np.zeros((h, w), np.float32), np.zeros((h, w, 2), np.float32)
    v = z2.copy()
    v[1, 2] = (1.5, -0.25)
    ref = z2.copy()
    ref[1, 2] = (0.5, 0.25)
    mask = np.full((h, w), 0.5, np.float32)
    inv = np.float32(1.0) / np.float32(w * h)
    e = R.planes(z1 + 1, v, z2, z1, z2, inv, P, ref, mask, 2.0)
    # (((10 * (1 + 0.5)) * 0.5) * 2) / 12
    assert e[R.TEMP][1, 2] == np.float32(15.0) * inv and np.count_nonzero(e[R.TEMP]) == 1
    assert not R.planes(z1 + 1, v, z2, z1, z2, inv, P)[R.TEMP].any()          # flag == false
    assert not e[R.SSIM].any() and not e[R.UI].any()                            # value == 1, ui_axy == 0


def test_sampling_known_answers():
    rng = np.random.RandomState(3)
    p = rng.rand(7, 9).astype(np.float32)
    assert np.array_equal(R.sample(p, 9, 7), p)                                 # ratio 1 copies
    c = np.full((7, 9), 0.375, np.float32)
    for w0, h0 in ((18, 14), (36, 7), (9, 28)):                                 # dyadic weights: every product is exact
        assert np.array_equal(R.sample(c, w0, h0), np.full((h0, w0), 0.375, np.float32))    # a constant plane stays constant
    for w0, h0 in ((23, 11), (4, 3)):                                           # any ratio: to the roundings of the blend
        assert np.allclose(R.sample(c, w0, h0), 0.375, rtol=8 * 2.0 ** -24, atol=0)
    # doubling a ramp in x: output pixel x sits at fx = x / 2 - 0.25, clamped taps at the borders
    r = np.tile(np.arange(4, dtype=np.float32), (2, 1))
    s = R.sample(r, 8, 2)
    assert np.array_equal(s[0], np.float32([0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3]))
    assert np.array_equal(s[0], s[1])
    # the plane is not rescaled by the size ratio
    assert abs(float(R.sample(c, 90, 70).max()) - 0.375) <= 0.375 * 8 * 2.0 ** -24      # ... not 3.75


def test_ramp_known_answers():
    t = np.float32([[-1.0, 0.0, 1.0 / 6, 1.0 / 3, 0.5, 2.0 / 3, 5.0 / 6, 1.0, 7.0]])
    rgb = R.ramp(t, 1.0)[0]
    assert rgb[0].tolist() == [0, 0, 0] and rgb[1].tolist() == [0, 0, 0]        # clamped at 0
    assert rgb[7].tolist() == [255, 255, 255] and rgb[8].tolist() == [255, 255, 255]   # clamped at 1
    assert rgb[2].tolist() == [128, 0, 0]                                       # 0.5 * 255 + 0.5 = 128.0
    assert rgb[3, 0] == 255 and rgb[3, 1] <= 1 and rgb[3, 2] == 0
    assert rgb[4].tolist() == [255, 128, 0]
    assert rgb[5, 0] == 255 and rgb[5, 1] == 255 and rgb[5, 2] <= 1
    assert rgb[6].tolist() == [255, 255, 128]
    # the gain scales before the clamp
    assert R.ramp(np.float32([[0.25]]), 2.0)[0, 0].tolist() == [255, 128, 0]
    assert R.ramp(np.float32([[0.25]]), 0.0)[0, 0].tolist() == [0, 0, 0]
    assert R.ramp(np.float32([[0.25]]), 100.0)[0, 0].tolist() == [255, 255, 255]
    assert R.image(np.full((3, 3), 0.5, np.float32), 5, 4, 1.0).shape == (4, 5, 3)
