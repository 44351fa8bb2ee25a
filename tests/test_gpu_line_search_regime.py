"""The control flow of the wave-wide golden-section search (decide64 of the FAST sweeps: initial pair, regime loop,
generic loop, final choice -- profiles/line_search_regime.md) against the plain loop.

vm_dbg_golden runs the search text the sweep kernels expand, a wave per case, on the energy
f(t) = (A (t - t0)) (t - t0) + B.  The reference is a numpy float32 statement of the generic loop as decide32 writes it:
one new point per step, xn = p R + q C as multiply, multiply, add, R = 0.618033989f, C = 1 - R, no regime, no
speculation.  The bits of tmin and fmin, the count of evaluations and the bits of every used point, in order, must be
equal for every case: the regime loop's collapsed bookkeeping (xn = b R, xn2 = xn R, `cc > eps`, shifts without a
select) and its hand-over to the generic loop change no bit and no count.

Cases (eps = 0.01): cc from [0, 10] plus exactly 0, eps, the next float above eps and 10 (no step; one step where the
guess-held check fails on cc alone; 15 steps), t0 in {0, inside (0, cc), cc, -1}, A in {1, -1, 0, 1e-3} (A = 0: every
comparison a tie), and one family with B = NaN (every comparison false: the search never leaves the regime)."""
import numpy as np
import pytest

from videomorphing_amd import capi

F = np.float32
EPS = F(0.01)
WORDS = 20          # per case: tmin, fmin, n_eval, 17 points


def make_cases():
    rng = np.random.RandomState(20260)
    ccs = np.concatenate([rng.uniform(0.0, 10.0, 200).astype(F),
                          np.array([0.0, EPS, np.nextafter(EPS, F(1)), 10.0], F)])
    rows = []
    for cc in ccs:
        inside = F(cc * F(rng.uniform(0.05, 0.95)))
        for t0 in (F(0), inside, cc, F(-1)):
            for A in (F(1), F(-1), F(0), F(1e-3)):
                rows.append((cc, A, t0, F(-0.25)))
        rows.append((cc, F(1), F(0), F(np.nan)))
    return np.array(rows, F)


def emulate(cc, A, t0, B):
    """the generic loop of decide32 in float32; returns (words of vm_dbg_golden's record, path class flags)"""
    R = F(0.618033989)
    C = F(1.0) - R

    def f(t):
        d = F(t - t0)
        return F(F(F(A * d) * d) + B)

    a = F(0)
    b = F(cc * C)
    x = F(F(b * R) + F(cc * C))
    fb, fx = f(b), f(x)
    pts = [b, x]
    regime_steps = other_steps = up_steps_with_a = 0
    in_regime = True                 # entered from the top only, left for good
    while F(cc - a) > EPS:
        lt = bool(fx < fb)
        if in_regime and not lt:
            assert a == 0
            regime_steps += 1
        else:
            in_regime = False
            other_steps += 1
            if not lt and a > 0:
                up_steps_with_a += 1
        p, q = (x, cc) if lt else (b, a)
        if lt:
            a = b
        else:
            cc = x
        xn = F(F(p * R) + F(q * C))
        fn = f(xn)
        pts.append(xn)
        if lt:
            b, x, fb, fx = x, xn, fx, fn
        else:
            b, x, fb, fx = xn, b, fn, fb
    lt = bool(fx < fb)
    tmin, fmin = (x, fx) if lt else (b, fb)
    rec = np.zeros(WORDS, np.uint32)
    rec[0] = np.array(tmin, F).view(np.uint32)
    rec[1] = np.array(fmin, F).view(np.uint32)
    rec[2] = len(pts)
    rec[3:3 + len(pts)] = np.array(pts, F).view(np.uint32)
    return rec, (regime_steps, other_steps, up_steps_with_a)


@pytest.fixture(scope="module")
def reference():
    cases = make_cases()
    with np.errstate(invalid="ignore"):
        out = [emulate(*row) for row in cases]
    return cases, np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def test_cases_cover_the_paths(reference):
    """a condition on the inputs: the mix walks every way through the two loops often enough to mean something"""
    cases, rec, cls = reference
    n = float(len(cases))
    reg, oth, up = cls[:, 0], cls[:, 1], cls[:, 2]
    never = np.sum((reg == 0) & (oth > 0)) / n
    stays = np.sum((reg > 0) & (oth == 0)) / n
    leaves = np.sum((reg > 0) & (oth > 0)) / n
    up_a = np.sum(up > 0) / n
    print("cases %d: never in the regime %.3f, in it throughout %.3f, enter and leave %.3f, an up-step with a > 0 %.3f; "
          "steps in the regime %.3f" % (n, never, stays, leaves, up_a, reg.sum() / float(reg.sum() + oth.sum())))
    assert 2000 <= n <= 8000
    assert never >= 0.05 and stays >= 0.05 and leaves >= 0.03 and up_a >= 0.03
    assert rec[:, 2].min() == 2 and rec[:, 2].max() == 17           # no step ... 15 steps
    nan_family = np.isnan(cases[:, 3])
    assert nan_family.sum() >= 200 and np.all(cls[nan_family, 1] == 0)      # NaN energies never leave the regime
    one_step = cases[:, 0] == np.nextafter(EPS, F(1))
    assert np.all(rec[one_step, 2] == 3) and np.all(rec[cases[:, 0] <= EPS, 2] == 2)


@pytest.mark.gpu
def test_the_two_loops_walk_the_plain_search(gpu_ctx, reference):
    cases, want, cls = reference
    n = len(cases)
    params = np.ascontiguousarray(cases, F)
    got = np.full((n, WORDS), 0xDEADBEEF, np.uint32)
    capi.check(gpu_ctx._L.vm_dbg_golden(gpu_ctx._h, n, params.ctypes.data, float(EPS), got.ctypes.data))
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    print("cases %d, differing %d" % (n, len(bad)))
    for k in bad[:8]:
        print("case", k, "cc A t0 B", cases[k], "class", cls[k], "\n got ", got[k], "\n want", want[k])
    assert np.array_equal(got[:, 2], want[:, 2])                   # evaluation counts
    assert np.array_equal(got[:, 3:], want[:, 3:])                 # the used points, in order
    assert np.array_equal(got[:, :2], want[:, :2])                 # tmin and fmin
