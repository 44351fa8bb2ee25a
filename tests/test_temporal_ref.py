"""tests/temporal_ref.py (the numpy statement of the temporal path) against the oracle, on the CPU, on every
case and shape of tests/temporal_cases.py:

  - the fixed-point statement equals the oracle bit for bit: the three accumulators, temp_ref, temp_mask and
    the in-between page of upsample();
  - the derived bound |from_fixed(acc) - S| <= n 2^-33 + |S| 2^-24 between the fixed-point accumulators and
    the exact (math.fsum) sums of the same contributions holds per pixel;
  - every case shows, on the oracle's output, what it was built to show -- a case that stopped exercising its
    edge fails here and never reaches a GPU.

Run with -s to see the figures quoted in tests/test_gpu_temporal_stages.py."""
import ctypes as C

import numpy as np
import pytest

import temporal_cases as TC
import temporal_ref as R

F32 = np.float32
CLAMPS = (0.0, 0.3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _oracle_acc(O, w, h, launches):
    """the oracle's accumulators after the given temp_ref launches [(v, fa, fb, ssim or None)]"""
    acc = np.zeros((h, w, 3), np.int64)
    for v, fa, fb, ssim in launches:
        a = [np.ascontiguousarray(x, dtype=F32) for x in (v, fa, fb)]
        s = np.ascontiguousarray(ssim, dtype=F32) if ssim is not None else None
        O.lib().vmo_temp_splat(w, h, *[x.ctypes.data for x in a], s.ctypes.data if s is not None else None, acc.ctypes.data)
    return acc


def oracle_initialize_temp(O, w, h, c, dr, clamp, seed=TC.SEED):
    """(temp_ref, temp_mask, value of the source page) of initialize_temp(dir) in the oracle"""
    v, fa, fb = TC.source(c, dr)
    src, dst = O.Level(w, h), O.Level(w, h)
    for k, lv in enumerate((src, dst)):
        lv.set_images(*TC.lumas(w, h, seed + k))
    src.field("v")[...] = v
    src.init(clamp)
    dst.init(clamp)
    dst.field("temp_ref")[...] = 0
    dst.field("temp_mask")[...] = 0
    dst.initialize_temp(src, fa, fb)
    return dst.field("temp_ref").copy(), dst.field("temp_mask").copy(), src.field("value").copy()


def oracle_fill(O, w, h, c):
    out = np.zeros((h, w, 2), F32)
    a = [np.ascontiguousarray(x, dtype=F32) for x in (c["v"][0], c["f0"], c["f1"], c["v"][1], c["b0"], c["b1"])]
    O.lib().vmo_temporal_fill(w, h, *[x.ctypes.data for x in a], out.ctypes.data)
    return out


def _assert_bound(acc, contribs, w, h):
    S, n = R.splat_f64(contribs, w, h)
    got = acc.astype(np.float64) / 4294967296.0
    got = got.astype(F32).astype(np.float64)
    assert (np.abs(got - S) <= R.fixed_sum_bound(S, n)).all()
    return n


@pytest.mark.parametrize("shape", TC.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_statement_equals_the_oracle_and_cases_show_their_edge(oracle, name, shape):
    w, h = shape
    c = TC.CASES[name](w, h, TC.SEED)
    fig = {}
    for dr in (-1, 1):
        v, fa, fb = TC.source(c, dr)
        for clamp in CLAMPS:
            ref_o, mask_o, value = oracle_initialize_temp(oracle, w, h, c, dr, clamp)
            con = R.Contributions(v, fa, fb, value)
            acc = R.splat_fixed([con], w, h)
            assert np.array_equal(acc, _oracle_acc(oracle, w, h, [(v, fa, fb, value)]))
            n = _assert_bound(acc, [con], w, h)
            ref_s, mask_s = R.initialize_temp(v, fa, fb, value, np.zeros((h, w, 2), F32), np.zeros((h, w), F32))
            assert np.array_equal(_bits(mask_s), _bits(mask_o)) and np.array_equal(_bits(ref_s), _bits(ref_o))
            TC.check_init(name, w, h, c, dr, ref_o, mask_o, value)
            if name == "noise":
                assert n.max() >= 6, n.max()
            if name == "rim":       # each rim is reached by footprints the frame cuts
                t = con.inside & con.cut
                assert ((con.tx == 0) & t).any() and ((con.tx == w - 1) & t).any()
                assert ((con.ty == 0) & t).any() and ((con.ty == h - 1) & t).any()
                prx, pry = con.p_ref
                assert ((prx >= -1) & (prx < 0)).any() and ((prx >= w - 1) & (prx < w)).any()
                assert ((pry >= -1) & (pry < 0)).any() and ((pry >= h - 1) & (pry < h)).any()
            if name in ("zero", "shift", "gaps"):      # whole-number landing positions: weights exactly 1 and 0
                assert set(np.unique(R.Contributions(v, fa, fb).fa)) <= {0.0, 1.0}
            if dr == -1 and clamp == 0.0:
                fig.update(init_holes=1 - (mask_o > 0).mean(), init_n=int(n.max()), init_w=float(mask_o.max()))
    # the in-between page of upsample()
    page_o = oracle_fill(oracle, w, h, c)
    cons = R.temporal_accumulate(c["v"][0], c["f0"], c["f1"], c["v"][1], c["b0"], c["b1"])
    acc = R.splat_fixed(cons, w, h)
    assert np.array_equal(acc, _oracle_acc(oracle, w, h, [(c["v"][0], c["f0"], c["f1"], None), (c["v"][1], c["b0"], c["b1"], None)]))
    n = _assert_bound(acc, cons, w, h)
    page_s, v_cur, weight = R.temporal_fill(c["v"][0], c["f0"], c["f1"], c["v"][1], c["b0"], c["b1"])
    assert np.array_equal(_bits(page_s), _bits(page_o))
    TC.check_fill(name, w, h, c, page_o)
    has = weight > 0
    left, right = R.nearest_weighted(weight)
    cols = np.broadcast_to(np.arange(w), (h, w))
    rows_with = has.any(1)
    if name == "zero":
        assert np.array_equal(_bits(v_cur), _bits(((c["v"][0] + c["v"][1]).astype(F32) / F32(2)))) and (weight == 2).all()
    if name == "shift":
        want = np.zeros((h, w), bool)
        want[:h - 2, 3:] = True
        assert np.array_equal(has, want)
        holes = ~has & rows_with[:, None]
        assert holes.any() and (right[holes] < w).all() and (left[holes] < 0).all()         # one-sided, all of them
    if name == "gaps":
        two = ~has & (left >= 0) & (right < w)
        assert two.any() and (two & (cols - left != right - cols)).any()
    if name == "converge":
        assert 1 <= has.sum() <= 9 and rows_with.sum() <= 3
        assert weight.max() >= 0.2 * w * h
        near = rows_with | np.roll(rows_with, 1) | np.roll(rows_with, -1)
        assert not _bits(page_o)[~near].any()
    if name == "leave":
        assert not acc.any()
    if name == "noise":
        assert n.max() >= 6
    if name in ("zero", "shift", "gaps"):
        assert all(set(np.unique(q.fa)) <= {0.0, 1.0} for q in cons)
    fig.update(fill_holes=1 - has.mean(), fill_n=int(n.max()), fill_w=float(weight.max()),
               empty_rows=int((~rows_with).sum()))
    print("\n%-9s %3dx%-3d initialize_temp(-1): holes %5.1f %%, <= %5d contributions, weight <= %9.3f | in-between page: "
          "holes %5.1f %%, <= %5d contributions, weight <= %9.3f, %3d rows without weight"
          % (name, w, h, 100 * fig["init_holes"], fig["init_n"], fig["init_w"], 100 * fig["fill_holes"], fig["fill_n"],
             fig["fill_w"], fig["empty_rows"]))


def test_fixed_point_rounds_to_nearest_even():
    """to_fixed at the ties of the 2^-32 grid and from_fixed's single rounding"""
    c = np.float32([2.0 ** -33, 3 * 2.0 ** -33, -(2.0 ** -33), 5 * 2.0 ** -33, 2.0 ** -34, 0.75, -1.5])
    assert R.to_fixed(c).tolist() == [0, 2, 0, 2, 0, 3 << 30, -(3 << 31)]
    assert R.from_fixed(np.int64([(1 << 32) + 1, 1 << 31])).tolist() == [1.0, 0.5]


def test_row_fill_by_hand():
    """fill_zeros_x on a row written out by hand: one-sided holes take v * d, two-sided ones
    (v_l + v_r) / (1 / d_l + 1 / d_r); a row without weight stays as it is"""
    wt = np.float32([[0, 0, 1, 0, 0, 0, 2, 0], [0] * 8])
    v = np.zeros((2, 8, 2), F32)
    v[0, 2], v[0, 6], v[1, 3] = (1, -2), (3, 5), (7, 7)
    out = R.fill_zeros_x(v, wt)
    assert out[0, :, 0].tolist() == [2, 1, 1, F32(4) / F32(1 + 1 / 3.0), 4, F32(4) / F32(F32(1 / 3.0) + 1.0), 3, 3]
    assert np.array_equal(out[1], v[1])
