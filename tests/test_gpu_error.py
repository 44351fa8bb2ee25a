"""The error view on the GPU, through the C-ABI (vm_level_energy, _energy_batch, _error_map, _error_image and the
vm_video_* three) against its numpy statement (tests/error_ref.py): planes and images bit for bit,
totals reproducible to the byte and within the summation bound of the exact sum, in EXACT within the statement's
bound of the oracle's vmo_energy.

Level sizes (each with a coarser level under it, BCOND_BORDER, three constraints, three sweeps): 9x7 one partial
workgroup; 67x33 width no multiple of 64, height no multiple of 4; 138x84 the smoke shape; 255x130 several workgroups
per row and a last-arriver fold over 132 partials in five ticket groups."""
import ctypes as C

import numpy as np
import pytest

import error_ref as R
from videomorphing_amd import capi, morph, synth

pytestmark = pytest.mark.gpu

MODES = [capi.MATH_EXACT, capi.MATH_FAST]
STATE = ("v", "value", "tps_b", "ui_axy", "ui_b", "luma", "mean", "var", "cross", "impmask")
WHATS = (capi.ERR_SSIM, capi.ERR_TPS, capi.ERR_UI, capi.ERR_TEMP, capi.ERR_ALL)


def _use(ctx, O, mode=None):
    """the parameters every case of this file runs with"""
    P = O.default_params(bcond=capi.BCOND_BORDER)
    kp = capi.KernParams()
    for f, _ in capi.KernParams._fields_:
        setattr(kp, f, getattr(P, f))
    ctx.set_params(kp)
    if mode is not None:
        ctx.set_math_mode(mode)
    return P


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _solve_level(ctx, w, h, frame=0, lo=None, P=None):
    """level w x h over a coarser one, initialised with three constraints, three sweeps; the oracle level `lo` (if
    given) is taken through the same steps"""
    i0, i1 = synth.make_pair(w, h, frame=frame)
    v0 = (0.8 * synth.displacement(w, h)).astype(np.float32)
    cons = R.constraints(w, h)
    pyr = morph.Pyramid(ctx)
    pyr.build_levels([(w, h), (max((w + 1) // 2, 5), max((h + 1) // 2, 5))])
    pyr.upload_luma(1, i0, i1)
    pyr[1].v = v0
    ca, n = morph._cons_array(cons)
    capi.check(pyr._L.vm_init_level(pyr._h, 0, w, h, ca, n))
    if lo is not None:
        lo.set_images(i0, i1)
        lo.field("v")[...] = v0
        lo.init(P.ssim_clamp)
        lo.splat(w, h, cons)
    for _ in range(3):
        pr = capi.Progress()
        capi.check(pyr._L.vm_optimize_level(pyr._h, 0, 1.0, None, 1, C.byref(pr)))
        if lo is not None:
            lo.optimize_iter(P)
    return pyr


def _statement(lv, P, temporal=False, factor_d=1.0):
    f = {n: lv.field(n) for n in ("value", "v", "tps_b", "ui_axy", "ui_b")}
    inv_wh = np.float32(1.0) / np.float32(lv.width * lv.height)
    ref, mask = (lv.field("temp_ref"), lv.field("temp_mask")) if temporal else (None, None)
    return R.planes(f["value"], f["v"], f["tps_b"], f["ui_axy"], f["ui_b"], inv_wh, P, ref, mask, factor_d)


def _energy(pyr, lvl=0):
    out = (C.c_double * 5)()
    capi.check(pyr._L.vm_level_energy(pyr._h, lvl, out))
    return np.array(out[:], dtype=np.float64)


def _map(pyr, what, pitch=0, fill=np.float32(-77.0)):
    lv = pyr[1]
    out = np.full((lv.height, pitch or lv.width), fill, dtype=np.float32)
    capi.check(pyr._L.vm_level_error_map(pyr._h, 0, what, out.ctypes.data, pitch))
    return out


_cases = {}


@pytest.fixture
def case(request, gpu_ctx, oracle):
    """(pyramid, oracle level or None, P, the statement's planes, a snapshot of the state), built once per shape and mode"""
    (w, h), mode = request.param
    P = _use(gpu_ctx, oracle, mode)
    key = (w, h, mode)
    if key not in _cases:
        lo = oracle.Level(w, h) if mode == capi.MATH_EXACT else None
        pyr = _solve_level(gpu_ctx, w, h, lo=lo, P=P)
        snap = {n: _bits(pyr[1].field(n)).copy() for n in STATE}
        _cases[key] = (pyr, lo, P, _statement(pyr[1], P), snap)
    return _cases[key]


ALL_CASES = [pytest.param((s, m), id="%dx%d-%s" % (s[0], s[1], "exact" if m == capi.MATH_EXACT else "fast")) for s in R.SHAPES for m in MODES]


@pytest.mark.parametrize("case", ALL_CASES, indirect=True)
def test_planes_equal_the_statement_bit_for_bit(case):
    pyr, _, _, want, _ = case
    lv = pyr[1]
    assert (lv.field("ui_axy") > 0).any() and (lv.field("ui_axy") == 0).any()
    for what in WHATS:
        got = _map(pyr, what)
        assert np.array_equal(_bits(got), _bits(want[what])), "plane %d: %d words differ" % (what, (_bits(got) != _bits(want[what])).sum())
        pitch = lv.width + 5                                          # a pitched destination: the padding is not written
        gp = _map(pyr, what, pitch)
        assert np.array_equal(_bits(gp[:, :lv.width]), _bits(want[what])) and (gp[:, lv.width:] == np.float32(-77.0)).all()
    assert not want[capi.ERR_TEMP].any()                              # a vm_pyr has no temporal term
    assert want[capi.ERR_SSIM].any() and want[capi.ERR_TPS].any() and want[capi.ERR_UI].any()


@pytest.mark.parametrize("case", ALL_CASES, indirect=True)
def test_totals_are_ordered_folds_of_the_planes(case, gpu_ctx, oracle):
    pyr, lo, P, want, _ = case
    lv = pyr[1]
    tot = _energy(pyr)
    exact = R.exact_totals(want)
    for k in WHATS:
        print("total %d: device %.17g fsum %.17g bound %.3g" % (k, tot[k], exact[k], R.sum_bound(want[k])))
        assert abs(tot[k] - exact[k]) <= R.sum_bound(want[k]), k
    assert tot.tobytes() == _energy(pyr).tobytes()                    # two calls: identical bytes
    # EXACT: the state is the oracle's bit for bit, so the totals agree with vmo_energy within the statement's bound
    if lo is not None:
        assert np.array_equal(_bits(lo.field("value")), _bits(lv.field("value")))
        e = lo.energy(P)
        for k in (capi.ERR_SSIM, capi.ERR_TPS, capi.ERR_UI):
            print("term %d: device %.17g oracle %.17g bound %.3g" % (k, tot[k], e[k], R.statement_bound(want[k])))
            assert abs(tot[k] - e[k]) <= R.statement_bound(want[k]), k
    # a second context on the same inputs: identical bytes
    ctx2 = morph.Context(0, gpu_ctx.math_mode)
    try:
        _use(ctx2, oracle)
        pyr2 = _solve_level(ctx2, lv.width, lv.height)
        assert np.array_equal(_bits(pyr2[1].field("value")), _bits(lv.field("value")))
        assert _energy(pyr2).tobytes() == tot.tobytes()
        del pyr2
    finally:
        ctx2.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h", R.SHAPES)
def test_batch_totals_are_the_single_calls_bytes(gpu_ctx, oracle, w, h, mode):
    _use(gpu_ctx, oracle, mode)
    pyrs = [_solve_level(gpu_ctx, w, h, frame=k) for k in range(5)]
    single = [_energy(p) for p in pyrs]
    assert len({s.tobytes() for s in single}) == 5                    # distinct pairs
    for n in (1, 3, 5):
        sel = pyrs[5 - n:]                                            # 5 - n: the pairs change their place in the batch
        arr = (C.c_void_p * n)(*[p._h for p in sel])
        out = (C.c_double * (5 * n))()
        capi.check(gpu_ctx._L.vm_level_energy_batch(arr, n, 0, out))
        got = np.array(out[:], dtype=np.float64).reshape(n, 5)
        for i in range(n):
            assert got[i].tobytes() == single[5 - n + i].tobytes(), (n, i)


def _image(pyr, what, gain, w0, h0, pitch=0):
    out = np.full((h0, pitch or 3 * w0), 0xA5, dtype=np.uint8)
    capi.check(pyr._L.vm_level_error_image(pyr._h, 0, what, gain, w0, h0, out.ctypes.data, pitch))
    return out


# every shape at ratio 1; the smoke shape also enlarged by a non-integer ratio and shrunk
IMAGE_CASES = [pytest.param(c.values[0], None, id=c.id + "-ratio1") for c in ALL_CASES]
IMAGE_CASES += [pytest.param(c.values[0], size, id="%s-%dx%d" % ((c.id,) + size)) for c in ALL_CASES if c.values[0][0] == (138, 84)
                for size in ((277, 169), (64, 40))]


@pytest.mark.parametrize("case,size", IMAGE_CASES, indirect=["case"])
def test_image_equals_the_statement_byte_for_byte(case, size):
    pyr, _, _, want, _ = case
    lv = pyr[1]
    w0, h0 = size or (lv.width, lv.height)
    for what in WHATS:
        # a gain that leaves part of the image saturated: twice the reciprocal of the plane's median magnitude
        med = float(np.median(np.abs(want[what][want[what] != 0]))) if want[what].any() else 1.0
        gain = float(np.float32(2.0 / med))
        ref = R.image(want[what], w0, h0, gain)
        got = _image(pyr, what, gain, w0, h0)
        assert np.array_equal(got.reshape(h0, w0, 3), ref), "what %d: %d bytes differ" % (what, (got.reshape(h0, w0, 3) != ref).sum())
        if what in (capi.ERR_SSIM, capi.ERR_ALL):
            assert 0 < (ref == 255).all(-1).mean() < 1                # partly saturated
        pitch = 3 * w0 + 7                                            # pitched output: the padding bytes stay
        gp = _image(pyr, what, gain, w0, h0, pitch)
        assert np.array_equal(gp[:, :3 * w0].reshape(h0, w0, 3), ref) and (gp[:, 3 * w0:] == 0xA5).all()


def _smooth_flow(rng, w, h, amp):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b, c, d = rng.uniform(0, 2 * np.pi, 4)
    fx = amp * np.sin(2 * np.pi * x / w + a) * np.cos(2 * np.pi * y / h + b) + 0.3 * amp
    fy = amp * np.cos(2 * np.pi * x / w + c) * np.sin(2 * np.pi * y / h + d) - 0.2 * amp
    return np.stack([fx, fy], -1).astype(np.float32)


@pytest.mark.parametrize("mode", MODES)
def test_video_pages_and_the_temporal_term(gpu_ctx, oracle, mode):
    """a depth-3 level of 96x64 over a depth-2 level (factor_d = 2), analytic flows, vm_video_solve with two
    iterations per level: the page solved first has no temporal term, the chained pages have the statement's"""
    P = _use(gpu_ctx, oracle, mode)
    levels = [(96, 64, 3), (48, 32, 2)]
    rng = np.random.RandomState(11)
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, [1, 2], 3)
    frames = synth.page_frames(levels, dev.factor_t)
    pyrs = [synth.build_pyramid(*synth.make_pair(96, 64, frame=t, amp=0.012 * 96), 2) for t in range(3)]
    for t in range(3):
        dev.upload_luma(0, t, *pyrs[frames[0][t]][0])
        dev.upload_flows(0, t, *[_smooth_flow(rng, 96, 64, 1.2) for _ in range(4)])
    L = dev._L
    out5 = (C.c_double * 5)()
    assert L.vm_video_energy(dev._h, 0, 1, out5) == capi.VM_E_STATE           # nothing initialised yet
    capi.check(L.vm_video_solve(dev._h, 2.0, 1.0, None, 0, None, 1, None))
    fd = dev.factor_d(0)
    assert fd == 2.0
    for page in range(3):
        pg = dev.pages[0][page]
        chained = page != 1
        want = _statement(pg, P, chained, fd)
        snap = {n: _bits(pg.field(n)).copy() for n in STATE + ("temp_ref", "temp_mask")}
        for what in WHATS:
            got = np.full((64, 96), -77.0, dtype=np.float32)
            capi.check(L.vm_video_error_map(dev._h, 0, page, what, got.ctypes.data, 0))
            assert np.array_equal(_bits(got), _bits(want[what])), (page, what)
        assert want[capi.ERR_TEMP].any() == chained                   # the first-solved page: all zero; a chained page: not
        capi.check(L.vm_video_energy(dev._h, 0, page, out5))
        tot = np.array(out5[:])
        exact = R.exact_totals(want)
        for k in WHATS:
            assert abs(tot[k] - exact[k]) <= R.sum_bound(want[k]), (page, k)
        assert (tot[capi.ERR_TEMP] > 0) == chained and (chained or tot[capi.ERR_TEMP] == 0.0)
        gain = float(np.float32(2.0 / np.median(np.abs(want[capi.ERR_ALL]))))
        img = np.zeros((40, 61, 3), dtype=np.uint8)
        capi.check(L.vm_video_error_image(dev._h, 0, page, capi.ERR_ALL, gain, 61, 40, img.ctypes.data, 0))
        assert np.array_equal(img, R.image(want[capi.ERR_ALL], 61, 40, gain))
        for n in snap:
            assert np.array_equal(snap[n], _bits(pg.field(n))), n
    assert L.vm_video_energy(dev._h, 1, 0, out5) == capi.VM_E_STATE           # the coarsest level
    for args in ((0, 3), (0, -1), (2, 0), (-1, 0)):
        assert L.vm_video_energy(dev._h, args[0], args[1], out5) == capi.VM_E_INVALID and L.vm_last_error()
    assert L.vm_video_energy(dev._h, 0, 0, None) == capi.VM_E_INVALID
    assert L.vm_video_error_map(dev._h, 0, 0, 5, img.ctypes.data, 0) == capi.VM_E_INVALID
    assert L.vm_video_error_map(dev._h, 0, 0, 0, None, 0) == capi.VM_E_INVALID
    assert L.vm_video_error_image(dev._h, 0, 0, 0, 1.0, 0, 40, img.ctypes.data, 0) == capi.VM_E_INVALID
    # the facade's three
    e = dev.pages[0][0].energy()
    capi.check(L.vm_video_energy(dev._h, 0, 0, out5))
    assert [e[k] for k in capi.ERR_NAMES] == list(out5)
    assert dev.pages[0][0].error_map(capi.ERR_TEMP).any() and dev.pages[0][0].error_image(30, 20).shape == (20, 30, 3)


def test_refusals(gpu_ctx, oracle):
    P = _use(gpu_ctx, oracle, capi.MATH_EXACT)
    w, h = 67, 33
    i0, i1 = synth.make_pair(w, h)
    pyr = morph.Pyramid(gpu_ctx)
    pyr.build_levels([(w, h), (34, 17)])
    pyr.upload_luma(1, i0, i1)
    pyr[1].v = (0.8 * synth.displacement(w, h)).astype(np.float32)
    L, H = pyr._L, pyr._h
    out5 = (C.c_double * 5)()
    plane = np.zeros((h, w), np.float32)
    rgb = np.zeros((h, w, 3), np.uint8)

    def all_four(lvl, want):
        arr = (C.c_void_p * 1)(H)
        for call in (lambda: L.vm_level_energy(H, lvl, out5), lambda: L.vm_level_energy_batch(arr, 1, lvl, out5),
                     lambda: L.vm_level_error_map(H, lvl, 0, plane.ctypes.data, 0),
                     lambda: L.vm_level_error_image(H, lvl, 0, 1.0, w, h, rgb.ctypes.data, 0)):
            assert call() == want
            assert want == capi.VM_OK or L.vm_last_error()            # every refusal leaves a message

    all_four(0, capi.VM_E_STATE)                                      # before vm_init_level
    all_four(1, capi.VM_E_STATE)                                      # the coarsest level
    capi.check(L.vm_init_level(H, 0, w, h, None, 0))
    snap = {n: _bits(pyr[1].field(n)).copy() for n in STATE}
    all_four(0, capi.VM_OK)
    for lvl in (-1, 2):
        all_four(lvl, capi.VM_E_INVALID)
    arr1 = (C.c_void_p * 1)(H)
    refused = [lambda: L.vm_level_energy(H, 0, None),
               lambda: L.vm_level_energy_batch(arr1, 1, 0, None),
               lambda: L.vm_level_energy_batch(arr1, 0, 0, out5),
               lambda: L.vm_level_error_map(H, 0, -1, plane.ctypes.data, 0),
               lambda: L.vm_level_error_map(H, 0, 5, plane.ctypes.data, 0),
               lambda: L.vm_level_error_map(H, 0, 0, None, 0),
               lambda: L.vm_level_error_map(H, 0, 0, plane.ctypes.data, w - 1),
               lambda: L.vm_level_error_image(H, 0, 7, 1.0, w, h, rgb.ctypes.data, 0),
               lambda: L.vm_level_error_image(H, 0, 0, 1.0, 0, h, rgb.ctypes.data, 0),
               lambda: L.vm_level_error_image(H, 0, 0, 1.0, w, -3, rgb.ctypes.data, 0),
               lambda: L.vm_level_error_image(H, 0, 0, 1.0, w, h, None, 0),
               lambda: L.vm_level_error_image(H, 0, 0, 1.0, w, h, rgb.ctypes.data, 3 * w - 1)]
    msgs = set()
    for call in refused:                                              # one at a time: vm_last_error holds the latest only
        assert call() == capi.VM_E_INVALID
        msgs.add(L.vm_last_error())
    assert len(msgs) >= 8 and all(msgs)                               # each with a message of its own
    # pyramids of a batch must share their geometry
    other = morph.Pyramid(gpu_ctx)
    other.build_levels([(w + 1, h), (34, 17)])
    assert L.vm_level_energy_batch((C.c_void_p * 2)(H, other._h), 2, 0, (C.c_double * 10)()) == capi.VM_E_INVALID
    capi.check(L.vm_level_clear(H, 0))
    all_four(0, capi.VM_E_STATE)                                      # after vm_level_clear
    with pytest.raises(capi.VmError) as e:
        pyr[1].energy()
    assert e.value.code == capi.VM_E_STATE
    for n in snap:
        assert np.array_equal(snap[n], _bits(pyr[1].field(n))), n


def test_matching_thread_energies(gpu_ctx, oracle):
    gpu_ctx.set_math_mode(capi.MATH_EXACT)                            # bit-identical to the oracle, so two solves agree to the bit
    w, h = 138, 84
    i0, i1 = synth.make_pair(w, h)
    prm = morph.Parameters()
    prm.max_iter, prm.max_iter_drop_factor, prm.start_res, prm.bcond = 4, 1.0, 16, capi.BCOND_BORDER
    for k in R.constraints(w, h):
        prm.add_point_pair(*[float(x) for x in k[:4]], weight=float(k[4]))
    pyr = morph.Pyramid(gpu_ctx)
    pyr.build(i0, i1, prm.start_res)
    t = morph.MatchingThread(prm, pyr, keep_state=True)
    assert t.energies == {}
    t.start()
    t.wait()
    solved = list(range(1, pyr.size() - 1))
    assert sorted(t.energies) == solved and len(solved) >= 2          # one entry per solved level
    for el in solved:
        assert t.energies[el] == pyr[el].energy()                     # read afterwards: the same bits
        assert set(t.energies[el]) == set(capi.ERR_NAMES) and t.energies[el]["ssim"] > 0 and t.energies[el]["temp"] == 0.0
    assert np.array_equal(pyr[1].error_map(capi.ERR_ALL), _statement(pyr[1], prm)[capi.ERR_ALL])
    assert pyr[1].error_image(w, h, capi.ERR_SSIM, 100.0).shape == (h, w, 3)
    # the reference's behaviour (the default): every level is cleared as it finishes -- the totals were taken before
    pyr2 = morph.Pyramid(gpu_ctx)
    pyr2.build(i0, i1, prm.start_res)
    t2 = morph.MatchingThread(prm, pyr2)
    t2.start()
    t2.wait()
    assert t2.energies == t.energies
    with pytest.raises(capi.VmError):
        pyr2[1].energy()


def test_state_is_unchanged_by_every_call_of_this_file():
    assert _cases
    for (w, h, mode), (pyr, _, _, _, snap) in _cases.items():
        for n in STATE:
            assert np.array_equal(snap[n], _bits(pyr[1].field(n))), (w, h, mode, n)
