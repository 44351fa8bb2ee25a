"""tests/mgb_ref.py -- the float64 statement of the compositor's multigrid-preconditioned CG that test_gpu_mgb_stages.py
compares the device with -- checked against itself and against the oracle (CPU only)."""
import numpy as np
import pytest

import mgb_ref
import mgb_stages as M


def _small_system(seed, w=12, h=9):
    """<= 12 x 9 unknowns with holes and a few ties"""
    rng = np.random.RandomState(seed)
    unk = rng.rand(h, w) > 0.15
    unk[3:5, 4:7] = False
    tie = (rng.rand(h, w) > 0.7).astype(float)
    tie[0, :] = 1                      # every component of the graph is tied somewhere: A is definite
    L0 = mgb_ref.level0(unk, tie)
    # drop unknowns cut off from every tie (A would be singular on them)
    reach = L0.unk & (L0.sc > 0)
    for _ in range(w * h):
        grow = reach.copy()
        grow[:, 1:] |= reach[:, :-1] & (L0.we > 0)
        grow[:, :-1] |= reach[:, 1:] & (L0.we > 0)
        grow[1:] |= reach[:-1] & (L0.ws > 0)
        grow[:-1] |= reach[1:] & (L0.ws > 0)
        if (grow == reach).all():
            break
        reach = grow
    return np.where(reach, True, False) & unk, tie


@pytest.mark.parametrize("seed,table", [(1, (1,)), (2, (1, 1, 2)), (3, (2,)), (4, (2, 1, 3))])
def test_dense_M_is_symmetric_positive_and_improves_the_condition(seed, table):
    unk, tie = _small_system(seed)
    lv = mgb_ref.hierarchy(mgb_ref.level0(unk, tie))
    assert len(lv) >= 2
    nu = mgb_ref.nu_levels(mgb_ref.sizes(unk.shape[1], unk.shape[0]), table)
    idx = np.argwhere(lv[0].unk)
    n = len(idx)
    Mi, A = np.zeros((n, n)), np.zeros((n, n))
    for j, (y, x) in enumerate(idx):
        e = np.zeros(unk.shape + (1,))
        e[y, x, 0] = 1
        Mi[:, j] = mgb_ref.cycle(lv, e, nu)[0][lv[0].unk][:, 0]
        A[:, j] = lv[0].apply(e)[lv[0].unk][:, 0]
    assert np.abs(A - A.T).max() == 0
    assert np.abs(Mi - Mi.T).max() <= 1e-12 * np.abs(Mi).max()
    assert np.linalg.eigvalsh(0.5 * (Mi + Mi.T)).min() > 0
    ev = np.linalg.eigvals(Mi @ A).real
    assert ev.min() > 0 and ev.max() / ev.min() < np.linalg.cond(A)


def test_two_sweeps_equal_two_applications_of_the_one_sweep_half_steps():
    unk, tie = _small_system(5, 40, 27)
    lv = mgb_ref.hierarchy(mgb_ref.level0(unk, tie))
    r = np.random.RandomState(6).randn(27, 40, 3) * lv[0].unk[..., None]
    for table in ((2,), (2, 1, 3)):
        nu = mgb_ref.nu_levels(mgb_ref.sizes(40, 27), table)
        assert np.array_equal(mgb_ref.cycle(lv, r, nu)[0], mgb_ref.half_steps(lv, r, nu))
    assert not np.array_equal(mgb_ref.cycle(lv, r, [2] * len(lv))[0], mgb_ref.cycle(lv, r, [1] * len(lv))[0])


def test_size_tail_and_nu_tables_equal_hand_computed_values():
    # 26 x 18: 468 + 117 + 35 cells, everything fits one workgroup
    assert mgb_ref.sizes(26, 18) == [(26, 18), (13, 9), (7, 5)]
    assert mgb_ref.tail_level(mgb_ref.sizes(26, 18)) == 0
    assert mgb_ref.nu_levels(mgb_ref.sizes(26, 18)) == [1, 1, 2]
    # 380 x 260: levels 3 .. 6 hold 1584 + 408 + 108 + 28 = 2128 cells; with level 2's 6175 they pass 5120
    sz = [(380, 260), (190, 130), (95, 65), (48, 33), (24, 17), (12, 9), (6, 5)]
    assert mgb_ref.sizes(380, 260) == sz
    assert mgb_ref.tail_level(sz) == 3
    assert mgb_ref.nu_levels(sz) == [1, 1, 2, 2, 2, 2, 2]
    assert mgb_ref.nu_levels(sz, (2, 1, 3)) == [2, 1, 2, 3, 3, 3, 3]      # cut to 2 above the tail only
    assert mgb_ref.nu_levels(sz, mgb_ref.NU_QPATH) == [1] * 7
    # 6 x 3400: levels 3 .. 6 hold 425 + 213 + 107 + 54 = 799 cells and join the tail one by one; level 2 (2 x 850 = 1700 cells,
    # 850 pairs) joins too: 799 + 1700 + level 1's 5100 would be 7599 > 5120 iterates, so level 1 stays out -- as its 2 x 1700 =
    # 3400 pairs > 3072 would have kept it out anyway
    sz = mgb_ref.sizes(6, 3400)
    assert sz == [(6, 3400), (3, 1700), (2, 850), (1, 425), (1, 213), (1, 107), (1, 54)]
    assert mgb_ref.tail_level(sz) == 2
    # a canvas of 3 x 1700 itself: everything below it is 2499 cells and would fit with its 5100 iterates beside (7599 > 5120: no);
    # and its 3400 pairs > 3072: the tail starts at level 1
    sz = mgb_ref.sizes(3, 1700)
    assert sz[:2] == [(3, 1700), (2, 850)] and mgb_ref.tail_level(sz) == 1
    assert mgb_ref.parse_nu("2,1,3") == (2, 1, 3) and mgb_ref.parse_nu("") == ()


def test_float64_pcg_reaches_the_oracles_solution(oracle):
    """ties the statement to the system the product solves: 96 x 64, ex 10"""
    w, h, ex = 96, 64, 10
    e0, e1, v = M.canvas_case(w + 2 * ex, h + 2 * ex, ex, 9)
    other = e1[ex:ex + h, ex:ex + w].copy()
    ref, _, _ = oracle.poisson_extend(e0, w, h, ex, other, v, 1, tol=1e-9)
    filled, typ, _ = oracle.poisson_prepare(e0, w, h, ex, other, v, 1)
    assert np.array_equal(typ, mgb_ref.classify(e0))
    B, X0 = mgb_ref.poisson_system(filled, typ)
    lv = mgb_ref.hierarchy(mgb_ref.level0_of_types(typ))
    N, hist, x = mgb_ref.pcg(lv, B, X0, mgb_ref.nu_levels(mgb_ref.sizes(w + 2 * ex, h + 2 * ex)), 1e-9)
    assert 0 < N < 20 and hist[-1] <= 1e-9
    unk = typ > 0
    d = np.abs(np.clip(x, 0, 255)[unk] - ref[..., :3][unk].astype(float))
    assert d.max() <= 1.0, d.max()


def test_tolerance_rule():
    a = np.array([[1.0, -4.0]])
    bound, dev = mgb_ref.tolerance(a, a.astype(np.float32))
    assert dev == 0 and bound == 16 * np.finfo(np.float32).eps * 4
    bound, dev = mgb_ref.tolerance(a, (a + [[0, 4e-3]]).astype(np.float32))
    assert abs(dev - 1e-3) < 1e-6 and abs(bound - 8 * dev * 4) < 1e-9


@pytest.mark.parametrize("case", M.ITERATION_TABLE, ids=lambda c: "%s-%dx%d-%g" % (c[0], c[1], c[2], c[6]))
def test_iteration_table_is_the_statements(oracle, case):
    """the table test_gpu_mgb_stages.py holds the device to, re-derived: N is the float64 count, rel[N] <= tol / 2, rel[N - 1] >=
    2 tol, and the float32 run of the statement stops at the same N"""
    kind, w, h, ex, seed, side, tol, N = case
    if kind == "poisson":
        h64, h32 = (M.poisson_reference(oracle, w, h, ex, seed, side, dt, tol) for dt in (np.float64, np.float32))
    else:
        h64, h32 = (M.qpath_reference(oracle, w, h, ex, seed, dt, tol) for dt in (np.float64, np.float32))
    assert M.safe_count(h64, h32, tol) == N, (h64, h32)
