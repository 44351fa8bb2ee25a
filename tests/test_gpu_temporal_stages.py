"""The temporal coherence path stage by stage, at its edges (the cases and shapes of tests/temporal_cases.py), and the
flag == true energy term under every sweep schedule on drawn levels.  Every comparison is an equality of bits:

  (a) vm_video_initialize_temp against the oracle, every case x shape, both directions, ssim_clamp 0 and 0.3
  (b) vm_video_upsample with depth doubling (5 <- 3 and 4 <- 2 pages) against the oracle, every case x shape
  (c) EXACT sweeps with the term against the oracle: TILE, SPLIT, STEP, SPARSE and PASS on drawn levels
      (w_temp over three decades, factor_d 1 / 2 / 4, the cases' masks, constraints, boundary conditions)
  (d) FAST sweeps with the term: STEP and PASS against SPLIT, SPARSE against TILE, state and counters
  (e) a pyramid whose second level is the largest: the temporal scratch is sized by the largest level

The oracle's own parity with a numpy statement of upsample.cu, the derived bound of its fixed-point sums and the
conditions every case must show are tests/test_temporal_ref.py (CPU).

What the cases show in the oracle (tests/test_temporal_ref.py -s; initialize_temp(dir = -1) with ssim_clamp 0 | the
in-between page of upsample(); hole share, largest number of contributions to one pixel, largest accumulated weight):

    case      shape     holes  contrib.  weight  |  holes  contrib.   weight   rows without weight
    zero      257x131    0.0 %      4     0.922  |   0.0 %      8      2.000     0
    shift     257x131    2.7 %      4     0.913  |   2.7 %      8      2.000     2
    shift       5x5     76.0 %      4     0.156  |  76.0 %      8      2.000     2
    gaps      257x131    2.3 %      4     0.907  |   2.0 %      8      2.000     0
    gaps       33x37    18.2 %      4     0.722  |  16.1 %      8      2.000     0
    converge  257x131  100.0 %  33667  8589.043  | 100.0 %  67334  26301.299   129
    converge   33x37    99.7 %   1221   352.152  |  99.7 %   2442    954.200    35
    leave     257x131  100.0 %      0     0      | 100.0 %      0      0       131
    rim       257x131   98.5 %    195    60.794  |  98.5 %    390    180.500     0
    far       257x131    0.1 %     10     2.049  |   0.0 %     15      4.608     0
    noise     257x131   25.3 %     20     3.837  |  23.8 %     35     10.246     0
    noise       5x5     20.0 %      9     0.589  |   4.0 %     18      4.600     0
    smooth_1  257x131    0.0 %      6     0.988  |   0.0 %     12      2.388     0
    smooth_4  257x131    1.1 %      8     1.161  |   0.3 %     12      2.642     0

That these tests can fail: arithmetic-only mutants of the library (none touches an index or a bound), each built on a
scratch copy and run once on this file.  Tests that failed (cases x shapes in brackets; (a) has 90, (b) 90 + 9):

    mutant                                               (a)   (b)   (b) leak  (c)   (d) STEP/PASS  (d) SPARSE  (e) stages  (e) solve
    k_temp_finish: wt >= 0 for wt > 0                     76     -      -      2/2       -             -           x           x
        (all cases with a hole: 0 / 0 is written to temp_ref where nothing landed; `zero` has none)
    k_temp_splat: weight product in float, not double     45    36     9/9     2/2       -             -           x           x
        (converge, far, noise, smooth_1, smooth_4: every case with fractional landing positions)
    to_fixed: truncation instead of round-to-nearest      50    26     6/9     2/2       -             -           x           x
    k_temp_splat: ssim factor dropped                     81     -      -      2/2       -             -           x           x
        (all of (a) but `leave`; upsample() has no ssim factor)
    k_fill_zeros_x: 1.0f / (px - x) formed in float        -    17     1/9      -        -             -           -           -
        (gaps, rim, noise, smooth_4: two-sided holes whose 1 / d_l + 1 / d_r rounds twice)
    k_smooth: weightless neighbours counted                -    56     9/9      -        -             -           x           x
        (every case with a hole)
    decide64 (PASS, wide STEP; FAST): factor_d dropped     -     -      -       -       2/2            -           -           -
    energy_x32 (STEP, PASS; EXACT): factor_d dropped       -     -      -      2/2       -             -           -           x
    lean SPARSE loader: c.tmask = 1                        -     -      -       -        -            1/2          -           -

No mutant passes everything.  ((d) SPARSE ran with the seeds 91 and 92 then; 92, in whose draws the SPARSE kernel runs
once only, failed its own "the kernel really ran" check with and without every mutant and was replaced by 93, where it
runs in two of the six draws as under 91.  The lean loader's mutant was caught under seed 91.)
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from videomorphing_amd import capi, morph, synth
import temporal_cases as TC
import test_temporal_ref as TR

pytestmark = pytest.mark.gpu

F32 = np.float32
STATE = ("v", "luma", "mean", "var", "cross", "value", "tps_b", "ui_b", "impmask")
FLOWS = ("f0", "f1", "b0", "b1")
_ids = dict(ids=lambda s: "%dx%d" % s)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _kp(ctx, O, **kw):
    P = O.default_params(**kw)
    kp = capi.KernParams()
    for f, _ in capi.KernParams._fields_:
        setattr(kp, f, getattr(P, f))
    ctx.set_params(kp)
    return P


@functools.lru_cache(maxsize=None)
def _case(name, w, h, seed=TC.SEED):
    return TC.CASES[name](w, h, seed)


@functools.lru_cache(maxsize=None)
def _oracle_init(O, name, w, h, dr, clamp):
    return TR.oracle_initialize_temp(O, w, h, _case(name, w, h), dr, clamp)


# ---- (a) ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", TC.SHAPES, **_ids)
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_initialize_temp_equals_the_oracle(gpu_ctx, oracle, name, shape):
    """temp_ref and temp_mask of a page tied to its neighbour: dir = -1 reads the neighbour's f0 / f1, dir = +1 its
    b0 / b1; with ssim_clamp 0 and 0.3 (the weight's ssim factor at its floor).  A second call gives the same bits
    (the accumulation is order-independent and the scratch is cleared between calls); the case's condition holds on
    the device's result."""
    w, h = shape
    c = _case(name, w, h)
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels([(w, h, 2), TC.coarse_shape(w, h) + (2,)])
    L = dev._L
    for clamp in (0.0, 0.3):
        _kp(gpu_ctx, oracle, ssim_clamp=clamp)
        for dr in (-1, 1):
            page, src = (1, 0) if dr < 0 else (0, 1)
            dev.upload_luma(0, src, *TC.lumas(w, h, TC.SEED))
            dev.upload_luma(0, page, *TC.lumas(w, h, TC.SEED + 1))
            dev.upload_flows(0, src, *[c[k] for k in FLOWS])
            dev.pages[0][src].v = TC.source(c, dr)[0]
            dev.pages[0][page].v = np.zeros((h, w, 2), F32)
            capi.check(L.vm_video_init_level(dev._h, 0, None, 0))
            ref_o, mask_o, value_o = _oracle_init(oracle, name, w, h, dr, clamp)
            assert _same(value_o, dev.pages[0][src].field("value"))
            got = []
            for _ in range(2):
                capi.check(L.vm_video_initialize_temp(dev._h, 0, page, dr))
                got.append((dev.pages[0][page].field("temp_ref"), dev.pages[0][page].field("temp_mask")))
                assert _same(got[-1][1], mask_o), (clamp, dr)
                assert _same(got[-1][0], ref_o), (clamp, dr, np.abs(got[-1][0] - ref_o).max())
            TC.check_init(name, w, h, c, dr, got[0][0], got[0][1], value_o)


# ---- (b) ---------------------------------------------------------------------------------------------------------

def _load_upsample(vid, dev, name, w, h, d, ds):
    """flows of case `name` on every page of level 0 (seed + page), the case's own kind of v on the coarse pages"""
    cw, ch = TC.coarse_shape(w, h)
    per_page = [_case(name, w, h, TC.SEED + t) for t in range(d)]
    vid.set_flows(0, {k: [c[k] for c in per_page] for k in FLOWS})
    for t, c in enumerate(per_page):
        dev.upload_flows(0, t, *[c[k] for k in FLOWS])
    for i in range(ds):
        v = _case(name, cw, ch, TC.SEED + 10 + i)["v"][0]
        vid.pages[1][i].field("v")[...] = v
        dev.pages[1][i].v = v


def _upsampled(oracle, gpu_ctx, names, w, h, d, ds):
    """upsample(level 0 <- level 1) for the given cases in turn on ONE vm_video: the device's pages after the last"""
    levels = [(w, h, d), TC.coarse_shape(w, h) + (ds,)]
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, [1, 2])
    for name in names:
        vid = oracle.Video(levels)
        _load_upsample(vid, dev, name, w, h, d, ds)
        vid.upsample(0)
        capi.check(dev._L.vm_video_upsample(dev._h, 0))
        pages = [dev.pages[0][t].v for t in range(d)]
        for t in range(d):
            a = vid.pages[0][t].field("v")
            assert _same(a, pages[t]), (name, t, np.abs(a - pages[t]).max())
    return pages


@pytest.mark.parametrize("shape", TC.SHAPES, **_ids)
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_upsample_with_depth_doubling_equals_the_oracle(gpu_ctx, oracle, name, shape):
    """5 <- 3 pages (pages 1 and 3 splatted from both neighbours, smoothed, row-filled) and 4 <- 2 pages (the last odd
    page stays zero): every page of the destination level"""
    w, h = shape
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    _kp(gpu_ctx, oracle)
    # (the pages before and after come out of the spatial upsample here, so v is on no grid: the conditions of `shift`
    # and `gaps`, whose whole-number landing positions need the taps of a constant flow to be exact, are asserted on the
    # oracle in tests/test_temporal_ref.py and in (a) on the device)
    own = name in ("zero", "converge", "leave")
    pages = _upsampled(oracle, gpu_ctx, [name], w, h, 5, 3)
    for i in (1, 3):
        if own:
            TC.check_fill(name, w, h, dict(v=[pages[i - 1], pages[i + 1]]), pages[i])
    pages = _upsampled(oracle, gpu_ctx, [name], w, h, 4, 2)
    assert not _bits(pages[3]).any()
    if own:
        TC.check_fill(name, w, h, dict(v=[pages[0], pages[2]]), pages[1])


@pytest.mark.parametrize("shape", TC.SHAPES, **_ids)
def test_upsample_scratch_does_not_leak_between_pages(gpu_ctx, oracle, shape):
    """`leave` (nothing lands) and then `noise`, and the other way round, on one vm_video: a weight or accumulator left
    over from the previous page or call would show in the next"""
    w, h = shape
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    _kp(gpu_ctx, oracle)
    pages = _upsampled(oracle, gpu_ctx, ["leave", "noise", "leave"], w, h, 5, 3)
    assert not _bits(pages[1]).any() and not _bits(pages[3]).any()


# ---- (c), (d): the term in the sweeps -------------------------------------------------------------------------------

MASKS = ("gaps", "converge", "leave", "noise", "smooth_1", "smooth_4")
DEPTHS = ((3, 3), (3, 2), (5, 3, 2))          # factor_d of level 0: 1, 2, 4


def _draw(rng, trial, wmax, hmax, wmin=10, hmin=10):
    """a level of a video pyramid: size, kernel parameters incl. w_temp, 0 to 3 point constraints on the frames of its
    pages; the depth table and the case its flows (hence its temporal mask) come from go round with the trial, so that
    six trials hold every mask and every factor_d twice"""
    w, h = int(rng.randint(wmin, wmax)), int(rng.randint(hmin, hmax))
    depths = DEPTHS[(trial + trial // 3) % 3]
    name = MASKS[trial % len(MASKS)]
    kw = dict(bcond=int(rng.randint(0, 3)), w_tps=float(10 ** rng.uniform(-3, 0)), w_ssim=float(10 ** rng.uniform(0, 3)),
              w_ui=float(10 ** rng.uniform(3, 6)), ssim_clamp=float(rng.choice([0.0, 0.0, 0.3])),
              eps=float(rng.choice([0.01, 0.01, 0.003, 0.03])), w_temp=float(10 ** rng.uniform(-1, 2)))
    cons = []
    for _ in range(int(rng.randint(0, 4))):
        x, y = rng.uniform(2, w - 3), rng.uniform(2, h - 3)
        dx, dy = rng.uniform(-2, 2, size=2)
        cons.append((x - dx, y - dy, x + dx, y + dy, float(rng.choice([1.0, 0.5])), int(rng.randint(0, depths[0]))))
    levels = [(max(5, -(-w >> k)), max(5, -(-h >> k)), d) for k, d in enumerate(depths)]
    return dict(w=w, h=h, levels=levels, name=name, kw=kw, cons=np.float32(cons).reshape(-1, 6), seed=int(rng.randint(1 << 30)))


def _inputs(D):
    w, h, d = D["levels"][0]
    rng = np.random.RandomState(D["seed"])
    flows = [_case(D["name"], w, h, TC.SEED + t) for t in range(d)]
    lumas = [TC.lumas(w, h, t, noise_sigma=3.0) for t in range(d)]
    v0 = [(0.7 * synth.displacement(w, h, amp=1.0) + 0.1 * rng.randn(h, w, 2)).astype(F32) for _ in range(d)]
    return flows, lumas, v0


def _device_level(gpu_ctx, D, inputs):
    """level 0 of the draw on the device, initialised (constraints splatted), every page untied"""
    flows, lumas, v0 = inputs
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(D["levels"])
    for t in range(D["levels"][0][2]):
        dev.upload_luma(0, t, *lumas[t])
        dev.upload_flows(0, t, *[flows[t][k] for k in FLOWS])
        dev.pages[0][t].v = v0[t]
    carr, n = morph._vcons_array(D["cons"])
    capi.check(dev._L.vm_video_init_level(dev._h, 0, carr, n))
    return dev


def _oracle_level(O, D, inputs, P, sweeps):
    flows, lumas, v0 = inputs
    d = D["levels"][0][2]
    vid = O.Video(D["levels"])
    vid.set_flows(0, {k: [flows[t][k] for t in range(d)] for k in FLOWS})
    for t in range(d):
        vid.set_images(0, t, *lumas[t])
        vid.pages[0][t].field("v")[...] = v0[t]
    vid.init_level(0, P, D["cons"])
    its = vid.optimize_level(0, P, sweeps)
    return vid, [its[t] for t in range(d)]


def _sweep(dev, sweeps, fixed=0):
    d = len(dev.pages[0])
    prog = (capi.Progress * d)()
    capi.check(dev._L.vm_video_optimize_level(dev._h, 0, float(sweeps), None, fixed, prog))
    return prog


def _state(dev):
    return [[dev.pages[0][t].field(f) for f in STATE] for t in range(len(dev.pages[0]))]


EXACT_SCHEDULES = (capi.SWEEP_TILE, capi.SWEEP_SPLIT, capi.SWEEP_STEP, capi.SWEEP_SPARSE, capi.SWEEP_PASS)


@pytest.mark.parametrize("seed", [71, 72])
def test_exact_sweeps_with_the_term_equal_the_oracle_on_drawn_levels(gpu_ctx, oracle, seed):
    """EXACT, every schedule, 1-3 sweeps of every page of the level (the middle one untied, the others tied to their
    neighbour by initialize_temp): every state array and the per-page iteration counts equal oracle.Video.optimize_level;
    factor_d of 1, 2 and 4 all occur; and the term acted -- some page ends elsewhere than with w_temp = 0"""
    rng = np.random.RandomState(seed)
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    acted, factors, names = [], set(), set()
    try:
        for trial in range(8):
            D = _draw(rng, trial, 300, 120)
            sweeps = int(rng.randint(1, 4))
            inputs = _inputs(D)
            P = _kp(gpu_ctx, oracle, **D["kw"])
            vid, its = _oracle_level(oracle, D, inputs, P, sweeps)
            d = D["levels"][0][2]
            for sched in EXACT_SCHEDULES:
                gpu_ctx.set_tuning(sched, 0, 0)
                dev = _device_level(gpu_ctx, D, inputs)
                assert dev.factor_d(0) == vid.factor_d[1]
                prog = _sweep(dev, sweeps)
                assert [prog[t].iters for t in range(d)] == its, (trial, sched, D["w"], D["h"], D["name"])
                for t in range(d):
                    for f in STATE + ("temp_ref", "temp_mask"):
                        assert _same(vid.pages[0][t].field(f), dev.pages[0][t].field(f)), (trial, sched, t, f, D["w"], D["h"], D["name"], D["kw"])
            factors.add(dev.factor_d(0))
            names.add(D["name"])
            with_term = [dev.pages[0][t].v for t in range(d)]
            _kp(gpu_ctx, oracle, **dict(D["kw"], w_temp=0.0))
            dev = _device_level(gpu_ctx, D, inputs)
            _sweep(dev, sweeps)
            acted.append(any(not _same(with_term[t], dev.pages[0][t].v) for t in range(d)))
            if D["name"] == "leave":          # an all-zero mask: the term is there and adds nothing
                assert not acted[-1]
    finally:
        gpu_ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        _kp(gpu_ctx, oracle)
    print("the term changed the result in draws:", acted, "factor_d:", sorted(factors), "masks:", sorted(names))
    assert any(acted), acted
    assert factors == {1.0, 2.0, 4.0} and names == set(MASKS), (factors, names)


def _fast_run(gpu_ctx, D, inputs, sched, sweeps, resident=0, pruned=0, fixed=1):
    dev = _device_level(gpu_ctx, D, inputs)
    if pruned:              # into the pruned regime first, on the TILE schedule
        gpu_ctx.set_tuning(capi.SWEEP_TILE, 0, 0)
        _sweep(dev, pruned, 1)
    gpu_ctx.set_tuning(sched, 0, 0)
    gpu_ctx.set_sparse_resident(resident)
    prog = _sweep(dev, sweeps, fixed)
    d = len(dev.pages[0])
    return (_state(dev) + [[dev.pages[0][t].field(f) for f in ("temp_ref", "temp_mask")] for t in range(d)],
            [(prog[t].iters, prog[t].commits, prog[t].candidates, prog[t].evaluations, prog[t].active_tiles,
              prog[t].sched_launches[3]) for t in range(d)])


def _assert_runs_equal(a, b, counters, what):
    ca, cb = [[p[k] for k in counters] for p in a[1]], [[p[k] for k in counters] for p in b[1]]
    assert ca == cb, (what, ca, cb)
    for t, (pa, pb) in enumerate(zip(a[0], b[0])):
        for k, (x, y) in enumerate(zip(pa, pb)):
            assert _same(x, y), (what, t, k)


@pytest.mark.parametrize("seed", [81, 82])
def test_fast_step_and_pass_with_the_term_equal_split(gpu_ctx, oracle, seed):
    """FAST with the term: the STEP and PASS schedules against SPLIT, 1-6 sweeps: state of every page, commits, candidates
    and evaluations"""
    rng = np.random.RandomState(seed)
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    commits = 0
    try:
        for trial in range(8):
            D = _draw(rng, trial, 420, 160)
            sweeps = int(rng.randint(1, 7))
            inputs = _inputs(D)
            _kp(gpu_ctx, oracle, **D["kw"])
            runs = [_fast_run(gpu_ctx, D, inputs, s, sweeps) for s in (capi.SWEEP_SPLIT, capi.SWEEP_STEP, capi.SWEEP_PASS)]
            for k in (1, 2):
                _assert_runs_equal(runs[0], runs[k], (0, 1, 2, 3), (trial, k, D["w"], D["h"], D["name"], D["kw"], sweeps))
            commits += sum(p[1] for p in runs[0][1])
    finally:
        gpu_ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        gpu_ctx.set_sparse_resident(0)
        gpu_ctx.set_math_mode(capi.MATH_EXACT)
        _kp(gpu_ctx, oracle)
    assert commits > 1000, commits


@pytest.mark.parametrize("seed", [91, 93])
def test_fast_sparse_with_the_term_equals_tile(gpu_ctx, oracle, seed):
    """FAST with the term, from a pruned state (80 sweeps of TILE): 10-60 sweeps of SPARSE (resident visits automatic /
    re-centred at every commit / given up at the first) against TILE, fixed work and the reference's stopping rule:
    state of every page, iterations, commits, candidates, evaluations and active tiles"""
    rng = np.random.RandomState(seed)
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    used = 0
    try:
        for trial in range(6):
            D = _draw(rng, trial, 420, 200, 40, 40)
            if trial % 3:      # the reference's weights (the drawn ones often keep every pixel active)
                D["kw"] = {k: D["kw"][k] for k in ("bcond", "eps", "ssim_clamp", "w_temp")}
            sweeps, fixed = int(rng.randint(10, 60)), int(rng.randint(0, 2))
            inputs = _inputs(D)
            _kp(gpu_ctx, oracle, **D["kw"])
            runs = [_fast_run(gpu_ctx, D, inputs, s, sweeps, (0, 2, 3)[trial % 3], 80, fixed) for s in (capi.SWEEP_TILE, capi.SWEEP_SPARSE)]
            _assert_runs_equal(runs[0], runs[1], (0, 1, 2, 3, 4), (trial, D["w"], D["h"], D["name"], D["kw"], sweeps, fixed))
            assert not any(p[5] for p in runs[0][1])
            used += any(p[5] for p in runs[1][1])
    finally:
        gpu_ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        gpu_ctx.set_sparse_resident(0)
        gpu_ctx.set_math_mode(capi.MATH_EXACT)
        _kp(gpu_ctx, oracle)
    assert used >= 2, used          # the sparse kernel really ran


# ---- (e) a pyramid whose second level is the largest ------------------------------------------------------------------

def _pair(oracle, gpu_ctx, levels, factor_t, name="smooth_4", seed=5):
    """the same video on both sides: lumas of every page and the case's flows, every level with images"""
    vid = oracle.Video(levels)
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, factor_t)
    for l, (w, h, d) in enumerate(levels[:-1]):
        per_page = [_case(name, w, h, seed + t) for t in range(d)]
        vid.set_flows(l, {k: [c[k] for c in per_page] for k in FLOWS})
        for t in range(d):
            i0, i1 = TC.lumas(w, h, t, noise_sigma=1.0)
            vid.set_images(l, t, i0, i1)
            dev.upload_luma(l, t, i0, i1)
            dev.upload_flows(l, t, *[per_page[t][k] for k in FLOWS])
    return vid, dev


def test_temporal_stages_on_a_level_larger_than_the_finest(gpu_ctx, oracle):
    """levels (64, 40), (100, 70), (50, 35), (25, 18): level 1 has more pixels (and a longer pitch) than level 0.
    initialize_temp on level 1 and upsample into level 1 (5 <- 3 pages) work in the video's scratch"""
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    P = _kp(gpu_ctx, oracle)
    levels = [(64, 40, 5), (100, 70, 5), (50, 35, 3), (25, 18, 3)]
    vid, dev = _pair(oracle, gpu_ctx, levels, [1, 1, 2, 1])
    L = dev._L
    for i in range(3):
        v = _case("smooth_4", 50, 35, 40 + i)["v"][0]
        vid.pages[2][i].field("v")[...] = v
        dev.pages[2][i].v = v
    vid.upsample(1)
    capi.check(L.vm_video_upsample(dev._h, 1))
    for t in range(5):
        assert _same(vid.pages[1][t].field("v"), dev.pages[1][t].v), t
    assert np.abs(dev.pages[1][1].v).max() > 0.1
    vid.init_level(1, P)
    capi.check(L.vm_video_init_level(dev._h, 1, None, 0))
    for page, dr in ((3, -1), (1, +1), (4, -1), (0, +1)):
        src, fl = page + dr, vid.flows[1]
        fa, fb = (fl["f0"][src], fl["f1"][src]) if dr < 0 else (fl["b0"][src], fl["b1"][src])
        vid.pages[1][page].initialize_temp(vid.pages[1][src], fa, fb)
        capi.check(L.vm_video_initialize_temp(dev._h, 1, page, dr))
        assert _same(vid.pages[1][page].field("temp_mask"), dev.pages[1][page].field("temp_mask")), (page, dr)
        assert _same(vid.pages[1][page].field("temp_ref"), dev.pages[1][page].field("temp_ref")), (page, dr)
        assert (dev.pages[1][page].field("temp_mask") > 0).mean() > 0.8


def test_video_solve_on_a_level_larger_than_the_finest(gpu_ctx, oracle):
    """levels (64, 40), (100, 70), (50, 35), (25, 18) with depths 5, 5, 5, 3: level 2 is upsampled with depth doubling,
    levels 1 and 0 hold the same frames and are pipelined, each lane with accumulators of its own -- the larger level 1
    among them.  One vm_video_solve pipelined and one with VM_NO_VIDEO_PIPELINE=1: identical to each other and to the
    oracle's level-by-level walk from the device's coarse solution"""
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    P = _kp(gpu_ctx, oracle, w_temp=10.0)
    levels = [(64, 40, 5), (100, 70, 5), (50, 35, 5), (25, 18, 3)]
    vid, dev = _pair(oracle, gpu_ctx, levels, [1, 1, 1, 2])
    cons = np.float32([[20, 14, 23, 15, 1.0, 0], [40, 30, 38, 31, 1.0, 2], [12, 33, 14, 31, 0.8, 4]])
    carr, n = morph._vcons_array(cons)
    L = dev._L
    capi.check(L.vm_video_coarse_solve(dev._h, carr, n))
    for t in range(3):
        vid.pages[3][t].field("v")[...] = dev.pages[3][t].v
    for el in (2, 1, 0):
        vid.upsample(el)
        vid.init_level(el, P, cons)
        vid.optimize_level(el, P, 3.0)
    results = {}
    for mode in ("pipeline", "sequential"):
        if mode == "sequential":
            os.environ["VM_NO_VIDEO_PIPELINE"] = "1"
        try:
            prog = (capi.Progress * 15)()
            capi.check(L.vm_video_solve(dev._h, 3.0, 1.0, carr, n, None, 0, prog))
        finally:
            os.environ.pop("VM_NO_VIDEO_PIPELINE", None)
        results[mode] = ([[dev.pages[el][t].v.copy() for t in range(5)] for el in range(3)],
                         [[dev.pages[el][t].field("temp_mask") for t in range(5)] for el in range(2)],
                         [prog[k].iters for k in range(15)])
    for el in range(3):
        for t in range(5):
            assert _same(results["pipeline"][0][el][t], vid.pages[el][t].field("v")), (el, t)
            assert _same(results["pipeline"][0][el][t], results["sequential"][0][el][t]), (el, t)
    for el in range(2):
        for t in range(5):
            assert _same(results["pipeline"][1][el][t], vid.pages[el][t].field("temp_mask")), (el, t)
            assert _same(results["pipeline"][1][el][t], results["sequential"][1][el][t]), (el, t)
    assert results["pipeline"][2] == results["sequential"][2] and min(results["pipeline"][2]) >= 1
    assert max(np.abs(v).max() for v in results["pipeline"][0][1]) > 0.2
