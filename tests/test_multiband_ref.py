"""tests/multiband_ref.py, the numpy statement of the multiband render calls (videomorphing_amd/csrc/vm_multiband.hip),
pinned without a GPU: constants are fixed points of reduce and expand, a weight of 0 or 1 reconstructs the plate, the table
of ones stays beside the plain blend, a hard seam reaches no further than 2 ** (L + 2) columns, a schedule of (0, 1) is the
uniform call, the Bands helpers build the tables they promise -- and the nine entry points are there and refuse a NULL
frame."""
import ctypes as C

import numpy as np
import pytest

import chain_ref
import multiband_ref as MB
import transit_ref
import warp_ref
from multiband_ref import SHAPES
from render_cases import field as _field, same_bits as _same
from videomorphing_amd import capi, morph
from videomorphing_amd.multiband import Bands

f32 = np.float32
shapes = pytest.mark.parametrize("w,h,L", SHAPES)
NAMES = ("vm_frame_render_multiband", "vm_frame_render_multiband_layers", "vm_frame_render_multiband_transition",
         "vm_frame_render_multiband_transition_layers")


def _tables(L):
    return [1.0] * (L + 1), [4.0] * L + [1.0]


def _integer_plates(w, h, seed, c=3):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, c)).astype(f32), rng.randint(0, 256, (h, w, c)).astype(f32)


def test_the_constants_are_the_headers():
    assert capi.MULTIBAND_MAX_LEVELS == MB.MAX_LEVELS == 8
    assert (capi.MB_G0, capi.MB_G1, capi.MB_MASK, capi.MB_OUT) == (MB.G0, MB.G1, MB.MASK, MB.OUT) == (0, 1, 2, 3)
    assert C.sizeof(capi.BandsStruct) == 4 + 4 * 9


def test_fold_reflects_without_repeating_the_edge():
    assert MB.fold(np.array([-2, -1, 0, 4, 5, 6]), 5).tolist() == [2, 1, 0, 4, 3, 2]
    assert MB.fold(np.array([-2, -1, 0, 1, 2, 3]), 2).tolist() == [0, 1, 0, 1, 0, 1]      # the double fold at n = 2


@shapes
def test_a_constant_is_a_fixed_point_of_reduce_and_expand(w, h, L):
    """a constant byte-valued image comes back exactly: the weights 1/16 (1 4 6 4 1) and 1/8 (1 6 1), 1/2 (1 1) are dyadic"""
    for value in (0.0, 1.0, 37.0, 255.0):
        x = np.full((h, w, 3), f32(value))
        sizes = MB.level_sizes(w, h, L)
        for l in range(L):
            y = MB.reduce(x)
            assert y.dtype == f32 and y.shape == (sizes[l + 1][1], sizes[l + 1][0], 3) and np.all(y == f32(value))
            back = MB.expand(y, x.shape[1], x.shape[0])
            assert back.dtype == f32 and back.shape == x.shape and np.all(back == f32(value))
            x = y


@shapes
def test_a_weight_of_zero_or_one_returns_the_plate(w, h, L):
    """integer-valued plates, A = 0 (or 1) everywhere: c0 (or c1) exactly, under the table of ones and under [4, ..., 4, 1]
    (every sharp[l] >= 1, so m is 0 or 1 on every band)"""
    c0, c1 = _integer_plates(w, h, 3)
    for sharp in _tables(L):
        for a, want in ((0.0, c0), (1.0, c1)):
            got = MB.multiband(c0, c1, np.full((h, w), f32(a)), sharp)
            assert got.dtype == f32 and float(np.abs(got - want).max()) == 0.0, (sharp, a)


@shapes
def test_the_table_of_ones_stays_beside_the_plain_blend(w, h, L):
    """the table of ones under a uniform weight a: every band is blended with the same a, so the sum is the plain blend to
    rounding.  Plates from warp_ref's maps on random canvases.  The statement's prototype deviated from chain_ref.blend by at
    most 4.6e-5 over the six shapes and a in {0.3, 0.5}; the bound is 2e-4, that figure with a fourfold margin for other
    shapes and inputs (on the canvases of this test the deviation is at most 6.1e-5, at 150 x 97).  After the rounding the
    bytes are never more than one level apart."""
    rng = np.random.RandomState(11)
    ex = 4
    e0, e1 = (morph.make_extended(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), ex) for _ in range(2))
    v, u = _field(w, h, "smooth", True)
    map0, map1 = warp_ref.sampling_maps(v, u, 0.4)[:2]
    c0, c1 = MB.canvas_plates(e0, e1, ex, map0, map1)
    for a in (0.3, 0.5):
        got = MB.multiband(c0, c1, np.full((h, w), f32(a)), [1.0] * (L + 1))
        want = chain_ref.blend(c0, c1, a, 1)
        worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print("w %d h %d L %d a %g: deviation %.3g" % (w, h, L, a, worst))
        assert worst <= 2e-4, (a, worst)
        plain = (want.astype(np.float64) + 0.5).astype(np.uint8)
        assert np.abs(chain_ref.bytes_of(got, True).astype(int) - plain.astype(int)).max() <= 1


def test_a_hard_seam_reaches_no_further_than_its_levels():
    """a hard mask at column w // 2 of 160 x 37 under L = 3: every column at least 2 ** (L + 2) = 32 from the seam has the
    bytes of the single plate (observed reach: 23 columns), under both tables; on constant plates 40 and 200 the row across
    the seam rises monotonically from 40 to 200"""
    w, h, L = 160, 37, 3
    seam, reach = w // 2, 2 ** (L + 2)
    A = np.zeros((h, w), f32)
    A[:, seam:] = 1
    c0, c1 = _integer_plates(w, h, 5)
    flat0, flat1 = np.full((h, w, 1), f32(40)), np.full((h, w, 1), f32(200))
    for sharp in _tables(L):
        got = chain_ref.bytes_of(MB.multiband(c0, c1, A, sharp), True)
        assert np.array_equal(got[:, :seam - reach + 1], c0[:, :seam - reach + 1].astype(np.uint8)), sharp
        assert np.array_equal(got[:, seam + reach - 1:], c1[:, seam + reach - 1:].astype(np.uint8)), sharp
        differs = np.nonzero((got != np.where(A[..., None] > 0, c1, c0).astype(np.uint8)).any(axis=(0, 2)))[0]
        print("sharp %r: the seam reaches columns %d..%d" % (sharp, differs.min(), differs.max()))
        row = chain_ref.bytes_of(MB.multiband(flat0, flat1, A, sharp), True)[h // 2, :, 0].astype(int)
        assert row[0] == 40 and row[-1] == 200 and np.all(np.diff(row) >= 0), (sharp, row)


@pytest.mark.parametrize("t", [0.0, 0.37, 1.0])
def test_the_uniform_schedule_is_the_uniform_call(t):
    """under the schedule (0, 1) with the linear ease the rates are t everywhere: the statement's inputs, hence the statement,
    are the uniform call's at geo_fa = color_fa = t"""
    w, h, L = 45, 27, 3
    v, u = _field(w, h, "smooth", True)
    su = MB.scheduled_inputs(v, u, None, None, t, transit_ref.EASE_LINEAR)
    un = MB.uniform_inputs(v, u, t, t)
    for a, b in zip(su, un):
        assert _same(a, b)
    c0, c1 = _integer_plates(w, h, 9, 2)
    sharp = Bands.sharpen(L, 4).sharp
    assert _same(MB.render_layers(c0, c1, su, sharp), MB.render_layers(c0, c1, un, sharp))


def test_a_nan_weight_counts_as_zero_and_a_nan_pixel_becomes_byte_zero():
    A = np.full((5, 9), f32(0.5))
    A[2, 4] = np.nan
    c0, c1 = _integer_plates(9, 5, 1)
    R = MB.multiband(c0, c1, A, [1.0, 1.0, 1.0])
    assert np.isfinite(R).all()                     # fmaxf / fminf: the NaN loses on every band
    R[0, 0, 0], R[0, 0, 1], R[0, 0, 2] = np.nan, -3.0, 300.0
    assert chain_ref.bytes_of(R, True)[0, 0].tolist() == [0, 0, 255]


def test_the_bands_helpers():
    assert Bands.linear(3).sharp == (1.0, 1.0, 1.0, 1.0) and Bands.linear(3).levels == 3
    s = Bands.sharpen(4, 4.0)
    assert s.levels == 4 and s.sharp[4] == 1.0 and s.sharp[0] == 4.0
    assert s.sharp == tuple(float(f32(4.0 ** ((4 - l) / 4))) for l in range(4)) + (1.0,)
    assert all(a > b for a, b in zip(s.sharp, s.sharp[1:]))
    # the deepest table whose coarsest level is still at least 2 x 2
    assert Bands.for_size(1920, 1080).levels == 5 and Bands.for_size(1920, 1080, 8).levels == 8
    assert Bands.for_size(9, 5).levels == 2 and Bands.for_size(9, 5).sharp == (1.0, 1.0, 1.0)      # 9 x 5 -> 5 x 3 -> 3 x 2
    assert Bands.for_size(3, 3).levels == 1 and Bands.for_size(2, 2).levels == 0
    assert Bands.for_size(1 << 14, 1 << 14, 99).levels == 8
    for w, h, L in SHAPES:
        assert min(MB.level_sizes(w, h, L)[-1]) >= 2 and Bands.linear(L).validate(w, h)
    st = Bands.sharpen(2, 9.0).struct()
    assert st.levels == 2 and list(st.sharp)[:3] == [9.0, 3.0, 1.0]
    for bad in (Bands([1.0]), Bands([1.0] * 10), Bands([1.0, 0.5]), Bands([np.inf, 1.0]), Bands([np.nan, 1.0])):
        with pytest.raises(ValueError):
            bad.validate()
    with pytest.raises(ValueError):
        Bands.linear(3).validate(9, 5)


def test_the_entry_points_exist(vmlib):
    for n in NAMES + tuple(n + "_dev" for n in NAMES) + ("vm_dbg_multiband_level",):
        assert n in capi.SYMBOLS, n
        assert hasattr(vmlib, n), "libvmorph_hip.so does not export %s" % n
    for n in NAMES:
        short = n[len("vm_frame_"):]
        assert callable(getattr(morph.Frame, short)) and callable(getattr(morph.Frame, short + "_dev"))
    assert callable(morph.Frame.multiband_level)


def test_a_null_frame_is_refused(vmlib):
    buf = C.create_string_buffer(64)
    ms = C.c_float(0)
    b = Bands.linear(1).struct()
    for n in NAMES:
        assert getattr(vmlib, n)(None, C.byref(b), 0.5, 0 if "transition" in n else 0.5, buf, 0) == capi.VM_E_INVALID
        assert (n + ":").encode() in vmlib.vm_last_error()
        assert getattr(vmlib, n + "_dev")(None, C.byref(b), 0.5, 0 if "transition" in n else 0.5, C.byref(ms)) == capi.VM_E_INVALID
        assert (n + "_dev:").encode() in vmlib.vm_last_error()
    assert vmlib.vm_dbg_multiband_level(None, 0, 0, buf) == capi.VM_E_INVALID
    assert b"vm_dbg_multiband_level:" in vmlib.vm_last_error()
