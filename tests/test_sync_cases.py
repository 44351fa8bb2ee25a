"""The oracle alone on the cases of the sync stage's edge tests (tests/sync_cases.py): every condition
tests/test_gpu_sync_edges.py leans on that needs no GPU.  If one of these fails, a case no longer reaches
the path it was built for -- fix the case, never the condition."""
import numpy as np
import pytest

import oracle
import sync_cases as sc

_bits = sc._bits


@pytest.mark.parametrize("case", sc.A_CASES, ids=sc.a_id)
def test_mode_cases_reach_their_launch_mode(case):
    """brick count, mode class, idle workgroups and ticket groups of each row, recomputed from the shape"""
    w, h, d = case.dims
    nb = -(-w // 32) * -(-h // 8) * -(-d // 8)
    g = sc.launch_geometry(case.dims)
    assert nb == case.nb == g["nb"] and g["self_mode"] == case.self_mode == (nb <= 512)
    if case.self_mode:
        assert g["fold_rounds"] == 2        # the fold's second round runs: more than 256 partials
    else:
        assert (g["idle"], g["groups"], g["last_group"]) == (case.idle, case.groups, case.last_group)
        assert g["groups"] > 1              # the one-group branch of the arrival cannot be reached in ticket mode
        assert 3 * nb > 1024                # nor the table-in-LDS templates of the ticket-mode kernel


def test_mode_cases_cover_the_boundary_and_the_partial_group():
    nbs = [c.nb for c in sc.A_CASES]
    assert 257 in nbs and 512 in nbs and 513 in nbs
    ticket = [c for c in sc.A_CASES if not c.self_mode]
    assert any(c.last_group < 32 for c in ticket) and any(c.idle > 0 for c in ticket)
    assert any(c.last_group == 32 and c.idle == 0 for c in ticket)
    assert any(sc.bricks(c.dims)[0] > 1 and c.dims[0] % 32 == 1 and c.dims[1] % 8 == 1 for c in ticket)   # one-voxel bricks


@pytest.mark.parametrize("case", sc.A_CASES, ids=sc.a_id)
def test_mode_cases_constrain_both_ends_of_the_brick_order(case):
    """thirteen constraints; the UI term is non-zero in the first brick along z and in the last"""
    w, h, d = case.dims
    cons = sc.mode_cons(case.dims)
    assert len(cons) == 13 and cons[-1] == (0, 0, 0, 2 * w - 1, 2 * h - 1, d - 1)
    assert all(0 <= c[0] < 2 * w and 0 <= c[3] < 2 * w and 0 <= c[1] < 2 * h and 0 <= c[4] < 2 * h and 0 <= c[2] < d and 0 <= c[5] < d
               for c in cons)
    ui = oracle.sync_ui(w, h, d, 2 * w, 2 * h, cons, 100.0)[0]
    last = 8 * (sc.bricks(case.dims)[2] - 1)
    assert ui[:8].any() and ui[last:].any()
    assert (ui != 0).mean() < 0.5           # and most voxels carry none


@pytest.mark.parametrize("case", sc.A_CASES, ids=sc.a_id)
def test_mode_cases_have_a_solution_worth_comparing(case):
    fields, k, res = sc.a_want(case.dims, "zero", 20)
    assert k == 21 and np.isfinite(res).all() and all(np.isfinite(f).all() for f in fields)
    assert all(np.abs(f).max() > 1e-3 for f in fields), [float(np.abs(f).max()) for f in fields]
    # the iteration counts differ in every component, so a pass too many or too few shows
    for a, b in zip(sc.A_MAX_ITER, sc.A_MAX_ITER[1:]):
        fa, fb = sc.a_want(case.dims, "zero", a)[0], sc.a_want(case.dims, "zero", b)[0]
        assert all(not np.array_equal(_bits(x), _bits(y)) for x, y in zip(fa, fb)), (a, b)
    # the inherited field is kept: the level adds to it
    inh = sc.a_want(case.dims, "inherited", 2)[0]
    assert all(np.abs(i - z).max() > 0.5 for i, z in zip(inh, sc.a_want(case.dims, "zero", 2)[0]))


@pytest.mark.parametrize("dims", sc.B_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_components_finish_at_different_iterations(dims):
    """z is done from two iterations on (its residual is below tol^2 and its bits stop changing) while x still moves"""
    assert sc.launch_geometry(dims)["self_mode"] == (dims == (33, 9, 1024))
    at = {mi: sc.b_want(dims, mi) for mi in (2, 4, sc.B_MAX_ITER)}
    assert np.array_equal(_bits(at[2][0][2]), _bits(at[sc.B_MAX_ITER][0][2]))
    assert 0 < at[2][2][2] < sc.B_DONE_BELOW and at[sc.B_MAX_ITER][2][2] == at[2][2][2]
    assert not np.array_equal(_bits(at[2][0][0]), _bits(at[4][0][0]))
    assert at[2][2][0] > sc.B_DONE_BELOW and at[2][2][1] > sc.B_DONE_BELOW
    assert np.abs(at[sc.B_MAX_ITER][0][2]).max() > 1e-3
    print(dims, [(mi, at[mi][2]) for mi in at])


def test_same_frame_constraints_leave_z_without_a_right_hand_side():
    w, h, d = sc.B_DIMS[0]
    ui = oracle.sync_ui(w, h, d, 2 * w, 2 * h, sc.same_frame_cons(sc.B_DIMS[0]), 100.0)
    assert ui[0].any() and ui[1].any() and ui[2].any() and not ui[3].any()


def test_workspace_sequence_alternates_the_modes():
    modes = [sc.launch_geometry(sc.C_LEVELS[lvl])["self_mode"] for lvl, _ in sc.C_STEPS]
    assert modes == [False, True, False]
    assert sc.nbricks(sc.C_LEVELS[2]) == 129
    a, b = sc.c_want(0), sc.c_want(2)
    assert a[1] == b[1] == sc.C_MAX_ITER + 1
    assert all(not np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[0], b[0]))     # a new field the second time


@pytest.mark.parametrize("shape", sc.D_SHAPES, ids=sc.shape_id)
def test_result_shapes_are_finite_and_reach_the_border_rules(shape):
    (w, h), (w0, h0) = shape
    f = sc.random_field((w, h, sc.D_DEPTH), 7000 + w + h)
    for z in range(sc.D_DEPTH):
        out = oracle.sync_result(f[0][z], f[1][z], f[2][z], w0, h0)
        assert np.isfinite(out).all() and np.abs(out[..., :3]).max() > 0.1 and not out[..., 3].any()


def test_result_shapes_cover_the_ratios():
    ratios = {(round(s[1][0] / s[0][0], 2), round(s[1][1] / s[0][1], 2)) for s in sc.D_SHAPES}
    assert (5.58, 5.62) in ratios and (1.0, 1.0) in ratios
    assert any(s[0][0] == 1 for s in sc.D_SHAPES) and any(s[0][1] == 1 for s in sc.D_SHAPES)
    assert any(r[0] > 30 for r in ratios)


@pytest.mark.parametrize("shape", sc.E_SHAPES, ids=sc.shape_id)
def test_upsample_shapes_are_finite(shape):
    (sw, sh), (dw, dh) = shape
    src = np.random.default_rng(1).standard_normal((sh, sw)).astype(np.float32)
    out = oracle.sync_upsample(src, dw, dh, sc.upsample_ratios(shape[0], shape[1])[0])
    assert out.shape == (dh, dw) and np.isfinite(out).all() and np.abs(out).max() > 0


@pytest.mark.parametrize("case", [c for c in sc.f_cases() if c[1] == "banded"], ids=sc.f_id)
def test_banded_inputs_take_every_branch_of_the_time_lookup(case):
    """|x|, |y| <= A; per band at least a tenth of the frame lies further than A + 1 from a band edge, and those
    pixels take the low clamp, the high clamp and the in-between branch with certainty"""
    shape, kind, layout = case
    w0, h0, d = shape
    rc = sc.render_case(shape, kind, layout)
    assert all(np.abs(rc.field[c]).max() <= sc.F_AMP for c in range(2)) and np.abs(rc.field[0]).max() > 0.5 * sc.F_AMP
    assert all(np.abs(f).max() <= sc.F_FLOW_AMP for f in rc.flows)
    inside = sc.band_interior(rc.bands)
    present = sorted(set(rc.bands.tolist()))
    assert present == ([0, 1, 2] if w0 >= sc.F_MIN_BAND else [layout])
    for b in present:
        assert (inside & (rc.bands == b)).sum() * h0 >= 0.1 * w0 * h0, (b, inside)
    z = rc.field[2]
    frac = z[:, :, rc.bands == 2]
    assert ((frac >= 0.2) & (frac <= 0.8)).all()
    assert (z[:, :, rc.bands == 0] == d + 1).all() and (z[:, :, rc.bands == 1] == -(d + 1)).all()
    # over both sides and the frames rendered, the bands present take these branches for certain
    taken = {sc.band_branch(b, d, f, s) for b in present for f in sc.f_frames(d) for s in (1, -1)}
    assert None not in taken
    if w0 >= sc.F_MIN_BAND:
        assert taken == ({"low", "high", "between"} if d > 1 else {"low", "high"})     # one frame: every time clamps


def test_banded_layouts_of_a_narrow_frame_cover_the_bands_in_turn():
    assert [int(l[0]) for l in sc.band_layouts(1)] == [0, 1, 2]
    got = set()
    for layout in range(3):
        got |= {sc.band_branch(layout, 1, 0, s) for s in (1, -1)}
    assert got == {"low", "high"}


@pytest.mark.parametrize("case", [c for c in sc.f_cases() if c[1] == "rough"], ids=sc.f_id)
def test_rough_inputs_are_finite_and_leave_the_image(case):
    shape, kind, layout = case
    w0, h0, d = shape
    rc = sc.render_case(shape, kind, layout)
    assert all(np.isfinite(a).all() for a in rc.field + rc.flows)
    y, x = np.mgrid[0:h0, 0:w0]
    if w0 > 1:
        for f in range(d):
            for s in (1, -1):
                px, py = x + s * rc.field[0][f], y + s * rc.field[1][f]
                assert (px < -1).any() and (px > w0).any() and (py < -1).any() and (py > h0).any()
    assert np.abs(rc.field[2]).max() <= sc.F_ROUGH_Z and (d == 1 or np.abs(rc.field[2]).max() > 1)


def test_render_cases_are_rendered_by_the_oracle():
    """the smallest and an odd-sized case end to end: finite inputs give bytes, and the field matters"""
    for shape, kind in (((1, 1, 1), "rough"), ((37, 11, 5), "banded"), ((37, 11, 5), "rough")):
        rc = sc.render_case(shape, kind)
        a = sc.render_want(rc, rc.field, 0.3, shape[2] // 2)
        assert a.shape == (shape[1], shape[0], 3) and a.dtype == np.uint8
        if shape[2] > 1:
            assert not np.array_equal(a, sc.render_want(rc, None, 0.3, shape[2] // 2))


def test_field_change_case():
    w0, h0, d = sc.G_LEVELS[0]
    cons = sc.g_cons()
    assert all(c[2] != c[5] for c in cons) and 0 < sc.G_FRAME < d - 1
    # the oracle's solve of level 1 moves the render of the frame under test
    w, h, _ = sc.G_LEVELS[1]
    f = [np.zeros((d, h, w), np.float32) for _ in range(3)]
    P = sc._params()
    oracle.sync_solve_level(f[0], f[1], f[2], w0, h0, cons, P.w_ui, P.w_tps, float(sc.G_MAX_ITER))
    rc = sc.g_case()
    zero = sc.render_want(rc, None, sc.G_FA, sc.G_FRAME)
    assert not np.array_equal(sc.render_want(rc, f, sc.G_FA, sc.G_FRAME), zero)
    f2 = sc.random_field(sc.G_LEVELS[2], 6300)
    assert not np.array_equal(sc.render_want(rc, f2, sc.G_FA, 0), sc.render_want(rc, None, sc.G_FA, 0))
