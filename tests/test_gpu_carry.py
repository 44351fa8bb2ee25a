"""Points and motion vectors through the morph on the GPU (videomorphing_amd/csrc/vm_carry.hip behind
vm_frame_carry_points, vm_frame_motion_maps and their forms under a schedule): bit for bit the float32
statement of tests/carry_ref.py, tied to the kernels that exist -- the dense call to the to-times {0, 1} is
vm_frame_sampling_maps, under a schedule vm_frame_transition_maps, the schedule (0, 1) gives the uniform bits -- and
refused in the stated order.

Shapes are those of the warp tests: 203x77 is no multiple of the 32x16 tile, 33x7 one partial tile narrower than the LDS
window, 5x3 smaller than the window's margin (every clamp), 138x84 the smoke shape; the large field's taps leave the
window, the field with NaN / Inf in it is compared NaN for NaN and bit for bit elsewhere (and must not fault)."""
import ctypes as C
import functools
import os
import textwrap

import numpy as np
import pytest

import carry_ref
from render_cases import field as _field, frame as _frame, hashes_under_render_mode, layers as _layers, same_bits as _same
from videomorphing_amd import capi, transition

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(203, 77, 9), (33, 7, 3), (5, 3, 2), (138, 84, 8)]
KINDS = ["smooth", "rough", "large", "shear", "outside", "nan"]
NAMES = ("out", "halfway", "pos0", "pos1", "resid", "flags")
cases = pytest.mark.parametrize("with_path", [False, True])


@functools.lru_cache(maxsize=None)
def _points(w, h):
    """257 start points, every species within the first 64: random sub-pixel points, pixel centres, points exactly on 0
    and w - 1 (h - 1), points up to +-2 w outside, 1e30, NaN and +-Inf"""
    rng = np.random.RandomState(5)
    p = (rng.rand(257, 2) * (w - 1, h - 1)).astype(f32)
    p[1:9] = [(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0), (0, 0.5 * (h - 1)), (w - 1, 1.25), (0.75, 0), (1.5, h - 1)]
    p[9:16] = [(1e30, 1), (2, -1e30), (np.nan, 1), (1, np.nan), (np.inf, 2), (0, -np.inf), (np.nan, np.inf)]
    p[16:32] = np.floor(p[16:32])                                               # pixel centres
    p[32:48] = (rng.rand(16, 2) * (4 * w, 4 * w) - (2 * w, 2 * w)).astype(f32)     # up to +-2 w outside
    p[128:160] = np.floor(p[128:160])
    p[160:200] = (rng.rand(40, 2) * (4 * w, 4 * w) - (2 * w, 2 * w)).astype(f32)
    p.setflags(write=False)
    return p


def _times(from_fa, nt):
    """the first nt of: 1.5, 0, the from-time, 1, -0.5, then 59 times across (0, 1)"""
    return ([1.5, 0.0, from_fa, 1.0, -0.5] + list(np.linspace(0.01, 0.99, 59)))[:nt]


def _all_same(got, want):
    return [k for k, g, r in zip(NAMES, got, want) if not _same(g, r)]


# ---- a. the points call
@pytest.mark.parametrize("w,h,ex", [SHAPES[0], SHAPES[2]])
@pytest.mark.parametrize("kind", KINDS)
@cases
def test_points_equal_the_statement(gpu_ctx, w, h, ex, kind, with_path):
    v, u = _field(w, h, kind, with_path)
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    froms = (0.0, 0.35, 1.0, 0.5)
    k = 0
    for n in (1, 64, 65, 257):
        for nt in (1, 3, 64):
            fa = froms[k % 4]
            k += 1
            pts, times = _points(w, h)[:n], _times(fa, nt)
            got = fr.carry_points(pts, fa, times)
            assert not _all_same(got, carry_ref.carry(v, u, pts, fa, times)), (n, nt, fa)
    fr.close()


@pytest.mark.parametrize("w,h,ex", [SHAPES[0], SHAPES[2]])
def test_each_output_alone_and_left_out(gpu_ctx, w, h, ex):
    """an output asked for alone, and every output but it: what comes back is what the full call gives"""
    v, u = _field(w, h, "rough", True)
    fr = _frame(gpu_ctx, w, h, ex, v, u, (transition.wipe(w, h, (1.0, 0.3), lead=0.6, duration=0.4), None))
    pts, times = _points(w, h)[:65], _times(0.35, 3)
    for call in (lambda **kw: fr.carry_points(pts, 0.35, times, **kw), lambda **kw: fr.carry_points_transition(pts, 0.35, times, 1, **kw)):
        full = call()
        for k, name in enumerate(NAMES):
            alone = call(want=(name,))
            assert _same(alone[k], full[k]) and all(a is None for j, a in enumerate(alone) if j != k), name
            rest = call(want=tuple(x for x in NAMES if x != name))
            assert rest[k] is None and all(_same(a, b) for j, (a, b) in enumerate(zip(rest, full)) if j != k), name
        timed = call(timed=True)
        assert timed[6] > 0 and all(_same(a, b) for a, b in zip(timed[:6], full))
    for call in (lambda **kw: fr.motion_maps(0.35, times, **kw), lambda **kw: fr.transition_motion_maps(0.35, times, 1, **kw)):
        full = call()
        for k, name in enumerate(("out", "resid", "flags")):
            alone = call(want=(name,))
            assert _same(alone[k], full[k]) and all(a is None for j, a in enumerate(alone) if j != k), name
            rest = call(want=tuple(x for x in ("out", "resid", "flags") if x != name))
            assert rest[k] is None and all(_same(a, b) for j, (a, b) in enumerate(zip(rest, full)) if j != k), name
    fr.close()


# ---- b. the dense call
@pytest.mark.parametrize("w,h,ex", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@cases
def test_motion_maps_equal_the_statement_and_the_sampling_maps(gpu_ctx, w, h, ex, kind, with_path):
    v, u = _field(w, h, kind, with_path)
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    grid = carry_ref.grid(w, h)
    for fa, nt in ((0.35, 1), (0.0, 3), (1.0, 16)):
        times = _times(fa, nt)
        out, resid, flags = fr.motion_maps(fa, times)
        want = carry_ref.carry(v, u, grid, fa, times)
        assert _same(out, want[0]) and _same(resid, want[4]) and _same(flags, want[5]), (fa, nt)
        # the points call on the grid is the dense call
        pout, _, _, _, presid, pflags = fr.carry_points(grid.reshape(-1, 2), fa, times)
        assert _same(pout.reshape(out.shape), out) and _same(presid.reshape(h, w), resid) and _same(pflags.reshape(h, w), flags)
    for fa in (0.0, 0.35, 1.0):
        out, resid, flags = fr.motion_maps(fa, [0.0, 1.0])
        m0, m1, r, fl = fr.sampling_maps(fa)
        # (as numbers: the closed form adds s2 * U = +-0 to the map)
        assert np.array_equal(out[0], m0, equal_nan=True) and np.array_equal(out[1], m1, equal_nan=True), fa
        assert _same(resid, r) and _same(flags, fl), fa
    assert fr.motion_maps_dev(0.35, _times(0.35, 3)) > 0
    fr.close()


_PROG = textwrap.dedent("""
    import hashlib, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import warp_ref
    from videomorphing_amd import capi, morph, synth, transition
    hh = hashlib.sha256()
    for w, h, ex in ((203, 77, 9), (33, 7, 3), (5, 3, 2)):
        rng = np.random.RandomState(41)
        v, u = warp_ref.field("rough", w, h, rng), warp_ref.path(w, h, rng)
        rgb0, rgb1 = synth.make_rgb_pair(w, h)
        fr = morph.Frame(morph.Context(0, capi.MATH_FAST), w, h, ex)
        for path in (None, u):
            fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, path)
            fr.upload_schedule(transition.wipe(w, h, (-1.0, 0.5), lead=0.7, duration=0.3), None)
            for a in fr.motion_maps(0.3, [0.0, 0.3, 1.0, 1.5]) + fr.transition_motion_maps(0.7, [0.1, 0.7, 1.2], 1):
                hh.update(a.tobytes())
    print("HASH", hh.hexdigest())
""") % (ROOT, os.path.join(ROOT, "tests"))


def test_plain_form_agrees(gpu_ctx):
    """the plain gather kernels (VM_RENDER=plain) give the window kernels' bits: a fresh child process with the switch
    set hashes the motion maps, uniform and scheduled, with and without a path; another one hashes the window form's"""
    assert hashes_under_render_mode(_PROG, "plain")[0] == hashes_under_render_mode(_PROG, None)[0]


# ---- c. under a schedule
@functools.lru_cache(maxsize=None)
def _schedule(w, h, name):
    if name == "wipe":
        s = transition.wipe(w, h, (1.0, 0.3), lead=0.6, duration=0.4)
    elif name == "radial":
        s = transition.radial(w, h, (0.3 * w, 0.6 * h), lead=0.5, duration=0.5)
    else:
        s = transition.wipe(w, h, (0.2, 1.0), lead=1.0, duration=0.0)         # a hard step: t1 == t0
        assert np.array_equal(s[..., 0], s[..., 1])
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("w,h,ex", [SHAPES[0], SHAPES[1]])
@pytest.mark.parametrize("name", ["wipe", "radial", "step"])
@cases
def test_transition_forms_equal_the_statement(gpu_ctx, w, h, ex, name, with_path):
    """points and dense, both eases, times before, inside and after the schedule; pos0 / pos1 / resid / flags on the grid
    are vm_frame_transition_maps'"""
    v, u = _field(w, h, "rough", with_path)
    sched = _schedule(w, h, name)
    fr = _frame(gpu_ctx, w, h, ex, v, u, (sched, None))
    grid = carry_ref.grid(w, h)
    pts = _points(w, h)[:65]
    times = [-0.5, 0.0, 0.2, 0.45, 0.8, 1.0, 1.7]
    for ease in (capi.EASE_LINEAR, capi.EASE_SMOOTH):
        for t in (-0.25, 0.3, 0.6, 1.4):
            got = fr.carry_points_transition(pts, t, times, ease)
            assert not _all_same(got, carry_ref.carry_transition(v, u, sched, pts, t, times, ease)), (ease, t)
        for t in (0.3, 1.4):
            want = carry_ref.carry_transition(v, u, sched, grid, t, times, ease)
            out, resid, flags = fr.transition_motion_maps(t, times, ease)
            assert _same(out, want[0]) and _same(resid, want[4]) and _same(flags, want[5]), (ease, t)
            got = fr.carry_points_transition(grid.reshape(-1, 2), t, times[:2], ease)
            m0, m1, r, fl, _ = fr.transition_maps(t, ease)
            assert _same(got[2].reshape(h, w, 2), m0) and _same(got[3].reshape(h, w, 2), m1), (ease, t)
            assert _same(got[4].reshape(h, w), r) and _same(got[5].reshape(h, w), fl) and _same(resid, r) and _same(flags, fl)
    assert fr.transition_motion_maps_dev(0.3, times) > 0
    fr.close()


@pytest.mark.parametrize("w,h,ex", [SHAPES[0], SHAPES[1]])
@cases
def test_uniform_schedule_gives_the_uniform_bits(gpu_ctx, w, h, ex, with_path):
    v, u = _field(w, h, "large", with_path)
    fr = _frame(gpu_ctx, w, h, ex, v, u, (transition.uniform(w, h), None))
    pts, times = _points(w, h), [0.0, 0.25, 0.6, 1.0]
    for fa in (0.0, 0.35, 1.0):
        assert not _all_same(fr.carry_points_transition(pts, fa, times, capi.EASE_LINEAR), fr.carry_points(pts, fa, times)), fa
        assert all(_same(a, b) for a, b in zip(fr.transition_motion_maps(fa, times, capi.EASE_LINEAR), fr.motion_maps(fa, times))), fa
    fr.close()


# ---- d. refusals
def test_refusals_in_the_stated_order_and_the_frame_unchanged(gpu_ctx):
    w, h, ex = 33, 7, 3
    v, u = _field(w, h, "rough", True)
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    fr.upload_layers(_layers(w, h, 2, 1), _layers(w, h, 2, 2))
    L, hnd = fr._L, fr._h
    INV, STATE = capi.VM_E_INVALID, capi.VM_E_STATE
    n, nt = 5, 2
    pts = np.ascontiguousarray(_points(w, h)[:n])
    to = f32([0.0, 1.0])
    bad_to = f32([0.0, np.nan])
    outs = [np.zeros((nt, n, 2), f32), np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.zeros(n, f32), np.zeros(n, np.uint8)]
    o = [a.ctypes.data for a in outs]
    none6 = [None] * 6
    dense = [np.zeros((nt, h, w, 2), f32), np.zeros((h, w), f32), np.zeros((h, w), np.uint8)]
    d = [a.ctypes.data for a in dense]
    ms = C.c_float(-1)
    P, T, B = pts.ctypes.data, to.ctypes.data, bad_to.ctypes.data

    def before():
        """v and the path as downloaded.  The facade downloads neither the layers nor the schedule: the layers are
        compared through what they render to, the schedule (further down, once the frame holds one) through the rates and
        maps of vm_frame_transition_maps -- the best there is"""
        return fr.download_v(), fr.download_qpath(), fr.render_layers(0.3, 0.35, 1)

    def unchanged(state):
        return all(_same(a, b) for a, b in zip(before(), state))

    state = before()
    # (the frame is compared after every group of refusals, and after every single call that goes through)
    # 1. the handle answers before anything else is looked at
    assert L.vm_frame_carry_points(None, np.nan, None, 0, None, 0, *none6, None) == INV
    assert L.vm_frame_motion_maps_dev(None, np.nan, None, 0, None) == INV
    # 2. NULL outputs and arrays answer before the arguments (n = 0, nt = 0, a NaN time, a bad ease are all there)
    for args in ((none6, P, T), (o, None, T), (o, P, None)):
        outs_, p_, t_ = args
        assert L.vm_frame_carry_points(hnd, np.nan, p_, 0, t_, 0, *outs_, C.byref(ms)) == INV
        assert L.vm_frame_carry_points_transition(hnd, np.nan, 7, p_, 0, t_, 0, *outs_, C.byref(ms)) == INV
    assert b"NULL" in L.vm_last_error()
    assert L.vm_frame_motion_maps(hnd, np.nan, T, 0, None, None, None) == INV and b"NULL" in L.vm_last_error()
    assert L.vm_frame_motion_maps(hnd, np.nan, None, 0, *d) == INV and b"NULL" in L.vm_last_error()
    assert L.vm_frame_transition_motion_maps(hnd, np.nan, 7, T, 0, None, None, None) == INV and b"NULL" in L.vm_last_error()
    assert L.vm_frame_motion_maps_dev(hnd, np.nan, None, 0, C.byref(ms)) == INV and b"NULL" in L.vm_last_error()
    assert L.vm_frame_transition_motion_maps_dev(hnd, np.nan, 7, None, 0, C.byref(ms)) == INV and b"NULL" in L.vm_last_error()
    assert unchanged(state)
    # 3. the arguments, before the state (this frame holds no schedule): n, nt, the from-time, a to-time, the ease
    for bad_n in (0, -3, (1 << 26) + 1, 2 ** 31 - 1):
        assert L.vm_frame_carry_points(hnd, 0.5, P, bad_n, T, nt, *o, None) == INV and b"points" in L.vm_last_error()
        assert L.vm_frame_carry_points_transition(hnd, 0.5, 0, P, bad_n, T, nt, *o, None) == INV
    for bad_nt in (0, 65, -1):
        assert L.vm_frame_carry_points(hnd, 0.5, P, n, T, bad_nt, *o, None) == INV and b"to-times" in L.vm_last_error()
        assert L.vm_frame_carry_points_transition(hnd, 0.5, 0, P, n, T, bad_nt, *o, None) == INV
    for bad_nt in (0, 17, 64):
        assert L.vm_frame_motion_maps(hnd, 0.5, T, bad_nt, *d) == INV and b"to-times" in L.vm_last_error()
        assert L.vm_frame_motion_maps_dev(hnd, 0.5, T, bad_nt, C.byref(ms)) == INV
        assert L.vm_frame_transition_motion_maps(hnd, 0.5, 0, T, bad_nt, *d) == INV
        assert L.vm_frame_transition_motion_maps_dev(hnd, 0.5, 0, T, bad_nt, C.byref(ms)) == INV
    for bad in (np.nan, np.inf, -np.inf):
        assert L.vm_frame_carry_points(hnd, bad, P, n, T, nt, *o, None) == INV and b"finite" in L.vm_last_error()
        assert L.vm_frame_carry_points_transition(hnd, bad, 0, P, n, T, nt, *o, None) == INV
        assert L.vm_frame_motion_maps(hnd, bad, T, nt, *d) == INV
        assert L.vm_frame_transition_motion_maps_dev(hnd, bad, 0, T, nt, C.byref(ms)) == INV
    assert L.vm_frame_carry_points(hnd, 0.5, P, n, B, nt, *o, None) == INV and b"finite" in L.vm_last_error()
    assert L.vm_frame_motion_maps(hnd, 0.5, B, nt, *d) == INV and b"finite" in L.vm_last_error()
    assert L.vm_frame_transition_motion_maps(hnd, 0.5, 0, B, nt, *d) == INV and b"finite" in L.vm_last_error()
    assert L.vm_frame_carry_points(hnd, np.nan, P, 0, T, nt, *o, None) == INV and b"points" in L.vm_last_error()     # n before the times
    assert L.vm_frame_carry_points(hnd, np.nan, P, n, T, 0, *o, None) == INV and b"to-times" in L.vm_last_error()    # nt before the times
    for ease in (-1, 2):
        assert L.vm_frame_carry_points_transition(hnd, 0.5, ease, P, n, T, nt, *o, None) == INV and b"ease" in L.vm_last_error()
        assert L.vm_frame_transition_motion_maps(hnd, 0.5, ease, T, nt, *d) == INV and b"ease" in L.vm_last_error()
        assert L.vm_frame_transition_motion_maps_dev(hnd, 0.5, ease, T, nt, C.byref(ms)) == INV
    assert L.vm_frame_carry_points_transition(hnd, np.nan, 2, P, n, T, nt, *o, None) == INV and b"finite" in L.vm_last_error()  # the times before the ease
    assert unchanged(state)
    # 4. the state
    assert L.vm_frame_carry_points_transition(hnd, 0.5, 0, P, n, T, nt, *o, None) == STATE
    assert L.vm_frame_transition_motion_maps(hnd, 0.5, 0, T, nt, *d) == STATE
    assert L.vm_frame_transition_motion_maps_dev(hnd, 0.5, 0, T, nt, C.byref(ms)) == STATE
    with pytest.raises(capi.VmError) as e:
        fr.carry_points_transition(pts, 0.5, [0.0])
    assert e.value.code == STATE
    assert all(not a.any() for a in outs + dense) and ms.value == -1      # nothing was written by a refused call
    assert unchanged(state)
    # the calls that go through leave the frame what it was, its schedule included
    sched = _schedule(w, h, "wipe")
    fr.upload_schedule(sched, sched)
    rates0 = fr.transition_maps(0.5, 1)
    capi.check(L.vm_frame_carry_points(hnd, 0.5, P, n, T, nt, *o, C.byref(ms)))
    assert ms.value > 0 and not _all_same(outs, carry_ref.carry(v, u, pts, 0.5, to))
    for call in (lambda: capi.check(L.vm_frame_carry_points(hnd, 0.5, P, n, T, nt, *o, None)),      # elapsed_ms may be NULL
                 lambda: fr.carry_points_transition(pts, 0.2, [0.9], 1),
                 lambda: fr.motion_maps(0.2, [0.9]),
                 lambda: fr.transition_motion_maps(0.2, [0.9], 1),
                 lambda: capi.check(L.vm_frame_motion_maps_dev(hnd, 0.5, T, nt, None)),
                 lambda: capi.check(L.vm_frame_transition_motion_maps_dev(hnd, 0.5, 1, T, nt, None))):
        call()
        assert unchanged(state) and all(_same(a, b) for a, b in zip(fr.transition_maps(0.5, 1), rates0))
    fr.clear_schedule()
    assert L.vm_frame_transition_motion_maps(hnd, 0.5, 0, T, nt, *d) == STATE
    fr.close()


def test_constraint_gaps(gpu_ctx):
    """the facade's gaps are the statement's; on a constant dyadic field they are exact"""
    w, h, ex = 33, 17, 2
    v = np.empty((h, w, 2), f32)
    v[...] = (3.5, -2.25)
    fr = _frame(gpu_ctx, w, h, ex, v, None)
    g01, g10, r01, r10 = fr.constraint_gaps([(10, 5, 17, 0.5, 1.0), (10, 5, 18, 0.5, 1.0)])
    assert g01.tolist() == [0.0, 1.0] and g10.tolist() == [0.0, 1.0] and not r01.any() and not r10.any()
    for none in (fr.constraint_gaps([]), carry_ref.constraint_gaps(v, None, [])):      # no constraints: four empty arrays
        assert len(none) == 4 and all(a.shape == (0,) and a.dtype == f32 for a in none)
    fr.close()
    w, h, ex = 203, 77, 9
    v, u = _field(w, h, "smooth", True)
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    cons = [capi.Constraint(20.5, 30.0, 24.0, 31.5, 1.0), capi.Constraint(150.0, 60.25, 149.0, 58.0, 0.5), capi.Constraint(0.0, 0.0, 202.0, 76.0, 1.0)]
    rows = [(c.lx, c.ly, c.rx, c.ry, c.weight) for c in cons]
    want = carry_ref.constraint_gaps(v, u, rows)
    assert all(_same(a, b) for a, b in zip(fr.constraint_gaps(cons), want))
    assert all(_same(a, b) for a, b in zip(fr.constraint_gaps(rows), want))
    fr.close()
