"""The synchronisation stage at the edges tests/test_gpu_sync.py does not reach, bit for bit (uint32 views,
bytes) against the oracle; cases in tests/sync_cases.py, their conditions proved on the CPU by
tests/test_sync_cases.py.

  A  level solves chosen by launch mode: SELF levels whose fold of the partials takes a second round (257 and
     512 bricks), ticket levels with idle workgroups and a last ticket group that is not full (513, 516, 522
     bricks), one with every group full (1024), each at 1, 2, 3 and 21 passes, from zero and from an inherited field
  B  a diagonal system (w_tps = 0) whose z component finishes after two iterations while x and y go on, in
     both modes; components that never start, in ticket mode
  C  one pyramid solving a ticket level, a SELF level and the ticket level again: stale tickets, partials and
     scalars in the kept workspace
  D  result delivery at production's ratio 5.58, at ratio 1, from one-column and one-row levels
  E  the level upsample from and to one-pixel-wide levels, with 1 and 5 pages
  F  the renderer on fields built to take the low clamp, the high clamp and the in-between branch of the
     time lookup, and on white noise that carries samples out of the image; d = 1 and 2; a padded output pitch
  G  what the renderer reads after the field changed under it

Not a gap: two of k_sync_A's six instantiations (the table-in-LDS ones of ticket mode) can never launch --
vm_sync_launch_iteration picks them for 3 nb <= 1024, ticket mode needs nb > 512 -- and neither can the
one-group branch of publish_and_arrive (ticket mode has at least 17 groups).  Nothing here looks for them."""
import ctypes as C

import numpy as np
import pytest

import oracle
import sync_cases as sc
from videomorphing_amd import capi, morph

_bits = sc._bits
_dims_id = lambda d: "%dx%dx%d" % d


def _same_bits(got, want, what):
    for c in range(3):
        assert np.array_equal(_bits(got[c]), _bits(want[c])), (what, "xyz"[c], float(np.abs(got[c] - want[c]).max()))


def _same_resid(pr, res):
    assert np.array_equal(_bits(np.array(pr.resid[:], np.float32)), _bits(res)), (pr.resid[:], res)


# ---- A ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", sc.A_MAX_ITER)
@pytest.mark.parametrize("kind", sc.A_KINDS)
@pytest.mark.parametrize("case", sc.A_CASES, ids=sc.a_id)
def test_level_solve_by_launch_mode(gpu_ctx, case, kind, max_iter):
    init = sc.a_init(case.dims, kind)
    got, pr, _ = sc._level_solve(gpu_ctx, sc.a_levels(case.dims), 1, sc.mode_cons(case.dims), sc._params(), max_iter, init=init)
    want, k, res = sc.a_want(case.dims, kind, max_iter)
    assert pr.iters == k == max_iter + 1 and pr.launches == 1 + 2 * pr.iters
    _same_bits(got, want, (case.dims, kind, max_iter))
    _same_resid(pr, res)


# ---- B ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dims", sc.B_DIMS, ids=_dims_id)
def test_a_component_that_finishes_mid_run(gpu_ctx, dims):
    """z is done after two iterations and is carried over unchanged for six more; x and y go on"""
    w, h, d = dims
    got, pr, _ = sc._level_solve(gpu_ctx, [(2 * w, 2 * h, d), dims], 1, sc.B_CONS, sc.b_params(), sc.B_MAX_ITER)
    want, k, res = sc.b_want(dims, sc.B_MAX_ITER)
    assert pr.iters == k and pr.launches == 1 + 2 * k
    _same_bits(got, want, dims)
    _same_resid(pr, res)
    assert 0 < pr.resid[2] < sc.B_DONE_BELOW


@pytest.mark.gpu
def test_ticket_mode_keeps_the_inherited_field_and_inactive_components(gpu_ctx):
    """tests/test_gpu_sync.py::test_level_solve_keeps_the_inherited_field_and_inactive_components on 516 bricks"""
    dims = sc.B_DIMS[0]
    w, h, d = dims
    levels = [(2 * w, 2 * h, d), dims]
    cons = sc.same_frame_cons(dims)
    P = sc._params()
    init = sc.random_field(dims, 7)
    got, pr, _ = sc._level_solve(gpu_ctx, levels, 1, cons, P, 30, init=init)
    want = [a.copy() for a in init]
    _, res = oracle.sync_solve_level(want[0], want[1], want[2], 2 * w, 2 * h, cons, P.w_ui, P.w_tps, 30.0)
    _same_bits(got, want, "same frames")
    assert np.array_equal(_bits(got[2]), _bits(init[2])) and res[2] == 0.0 and pr.resid[2] == 0.0
    _same_resid(pr, res)
    # no constraints at all: nothing moves
    got, pr, _ = sc._level_solve(gpu_ctx, levels, 1, [], P, 10, init=init)
    _same_bits(got, init, "no constraints")
    assert tuple(pr.resid[:]) == (0.0, 0.0, 0.0)


# ---- C ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_workspace_kept_between_levels(gpu_ctx):
    pyr = morph.SyncPyramid(gpu_ctx)
    pyr.build_levels(sc.C_LEVELS)
    P = sc._params()
    sc._set_cons(P, sc.c_cons())
    th = morph.SyncThread(P, pyr)
    th._max_iter = float(sc.C_MAX_ITER)
    for step, (lvl, seed) in enumerate(sc.C_STEPS):
        pyr.set_field(lvl, *sc.random_field(sc.C_LEVELS[lvl], seed))
        pr = th.optimize_level(lvl)
        want, k, res = sc.c_want(step)
        assert pr.iters == k and pr.launches == 1 + 2 * k
        _same_bits(pyr.field(lvl), want, ("step", step))
        _same_resid(pr, res)


# ---- D ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", sc.D_SHAPES, ids=sc.shape_id)
def test_result_delivery(gpu_ctx, shape):
    (w, h), (w0, h0) = shape
    d = sc.D_DEPTH
    f = sc.random_field((w, h, d), 7000 + w + h)
    pyr = morph.SyncPyramid(gpu_ctx)
    pyr.build_levels([(w0, h0, d), (w, h, d)])
    pyr.set_field(1, *f)
    for z in range(d):
        want = oracle.sync_result(f[0][z], f[1][z], f[2][z], w0, h0)
        assert np.array_equal(_bits(pyr.result(1, z)), _bits(want)), z


# ---- E ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pages", sc.E_PAGES)
@pytest.mark.parametrize("shape", sc.E_SHAPES, ids=sc.shape_id)
def test_upsample_level(gpu_ctx, vmlib, shape, pages):
    (sw, sh), (dw, dh) = shape
    pyr = morph.SyncPyramid(gpu_ctx)
    pyr.build_levels([(2 * dw, 2 * dh, pages), (dw, dh, pages), (sw, sh, pages)])
    src = sc.random_field((sw, sh, pages), 8000 + sw + dh)
    pyr.set_field(2, *src)
    capi.check(vmlib.vm_sync_upsample_level(pyr._h, 1))
    got = pyr.field(1)
    ratios = sc.upsample_ratios(shape[0], shape[1])
    for c in range(3):
        for z in range(pages):
            assert np.array_equal(_bits(got[c][z]), _bits(oracle.sync_upsample(src[c][z], dw, dh, ratios[c]))), (c, z)


# ---- F ---------------------------------------------------------------------------------------------

def _render_pyramid(ctx, shape, rc):
    """level 1 as large as level 0: the result resize copies the field through, so set_field states the vector"""
    pyr = morph.SyncPyramid(ctx)
    pyr.build_levels([shape, shape])
    sc.upload(pyr, rc)
    return pyr


@pytest.mark.gpu
@pytest.mark.parametrize("case", sc.f_cases(), ids=sc.f_id)
def test_render_resample_at_its_edges(gpu_ctx, case):
    shape, kind, layout = case
    rc = sc.render_case(shape, kind, layout)
    pyr = _render_pyramid(gpu_ctx, shape, rc)
    pyr.set_field(1, *rc.field)
    for frame in sc.f_frames(shape[2]):
        for fa in sc.F_FA:
            want = sc.render_want(rc, rc.field, fa, frame)
            got = pyr.render_resample(fa, frame)
            assert np.array_equal(got, want), (frame, fa, int(np.abs(got.astype(int) - want.astype(int)).max()),
                                               int((got != want).any(-1).sum()))


@pytest.mark.gpu
def test_render_with_padded_pitches(gpu_ctx, vmlib):
    shape = (37, 11, 5)
    w0, h0, d = shape
    rc = sc.render_case(shape, "rough")
    pyr = morph.SyncPyramid(gpu_ctx)
    pyr.build_levels([shape, shape])
    fp, lp = 4 * w0 + 8, 2 * w0 + 3        # bytes per frame row, floats per flow row
    for s in range(2):
        for t in range(d):
            frame = np.full((h0, fp), 0x5A, np.uint8)
            frame[:, :4 * w0] = rc.video[s][t].reshape(h0, 4 * w0)
            capi.check(vmlib.vm_sync_upload_frame(pyr._h, s, t, frame.ctypes.data, fp))
            flow = np.full((h0, lp), 1e30, np.float32)
            flow[:, :2 * w0] = rc.flows[s][t].reshape(h0, 2 * w0)
            capi.check(vmlib.vm_sync_upload_flow(pyr._h, s, t, flow.ctypes.data, lp))
    pyr.set_field(1, *rc.field)
    pitch = 3 * w0 + 5
    for fa, frame in ((0.3, 2), (0.999, d - 1)):
        out = np.full((h0, pitch), 0xA5, np.uint8)
        capi.check(vmlib.vm_sync_render(pyr._h, fa, frame, out.ctypes.data, pitch))
        want = sc.render_want(rc, rc.field, fa, frame)
        assert np.array_equal(out[:, :3 * w0].reshape(h0, w0, 3), want)
        assert (out[:, 3 * w0:] == 0xA5).all()


# ---- G ---------------------------------------------------------------------------------------------

def _g_pyramid(ctx):
    rc = sc.g_case()
    pyr = morph.SyncPyramid(ctx)
    pyr.build_levels(sc.G_LEVELS)
    sc.upload(pyr, rc)
    P = sc._params()
    sc._set_cons(P, sc.g_cons())
    th = morph.SyncThread(P, pyr)
    th._max_iter = float(sc.G_MAX_ITER)
    return rc, pyr, th


@pytest.mark.gpu
def test_render_after_the_first_solve_uses_the_solved_field(gpu_ctx):
    """a render before the solve (zero field), then load_identity + optimize_level as SyncThread drives them, then
    the same frame again"""
    rc, pyr, th = _g_pyramid(gpu_ctx)
    zero = sc.render_want(rc, None, sc.G_FA, sc.G_FRAME)
    assert np.array_equal(pyr.render_resample(sc.G_FA, sc.G_FRAME), zero)
    th.load_identity(1)
    th.optimize_level(1)
    want = sc.render_want(rc, pyr.field(1), sc.G_FA, sc.G_FRAME)
    assert not np.array_equal(want, zero)
    assert np.array_equal(pyr.render_resample(sc.G_FA, sc.G_FRAME), want)


@pytest.mark.gpu
def test_render_mid_solve_uses_the_level_last_delivered(gpu_ctx):
    """level 2 holds a field, level 1 none; update_result delivers every frame from level 2; a render of frame 0
    (not the frame delivered last) shows level 2's result"""
    rc, pyr, th = _g_pyramid(gpu_ctx)
    f2 = sc.random_field(sc.G_LEVELS[2], 6300)
    pyr.set_field(2, *f2)
    d = sc.G_LEVELS[0][2]
    for z in range(d):
        pyr.result(2, z)
    for frame in (0, d - 1):
        want = sc.render_want(rc, f2, sc.G_FA, frame)
        assert not np.array_equal(want, sc.render_want(rc, None, sc.G_FA, frame))
        assert np.array_equal(pyr.render_resample(sc.G_FA, frame), want), frame


@pytest.mark.gpu
def test_render_after_a_second_solve_uses_the_new_field(gpu_ctx):
    """result(1, f) delivered, then the level is solved again (the level adds to what it holds): the frame's
    cached vector is stale"""
    rc, pyr, th = _g_pyramid(gpu_ctx)
    th.load_identity(1)
    th.optimize_level(1)
    pyr.result(1, sc.G_FRAME)
    old = sc.render_want(rc, pyr.field(1), sc.G_FA, sc.G_FRAME)
    assert np.array_equal(pyr.render_resample(sc.G_FA, sc.G_FRAME), old)
    th.optimize_level(1)
    want = sc.render_want(rc, pyr.field(1), sc.G_FA, sc.G_FRAME)
    assert not np.array_equal(want, old)
    assert np.array_equal(pyr.render_resample(sc.G_FA, sc.G_FRAME), want)
