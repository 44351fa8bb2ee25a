"""tests/viewport_ref.py, the numpy statement of the viewport calls (videomorphing_amd/csrc/vm_viewport.hip), pinned without
a GPU to what exists: at the identity viewport its landing is warp_ref.sampling_maps bit for bit and its bytes are the
oracle's, an integer crop is the slice, the 2 x 2 box property holds byte for byte, a constant canvas gives the constant
under any viewport, the sample grid is symmetric about the pixel centre -- and the struct, the validator and the entry
points are what include/vmorph.h says."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import viewport_ref
import warp_ref
from videomorphing_amd import capi, morph, synth
from videomorphing_amd.viewport import Viewport

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(203, 77, 9), (33, 7, 0), (5, 3, 2)]        # tests/test_warp_ref.py's
NAMES = ("vm_render_viewport", "vm_render_viewport_dev", "vm_render_viewport_layers", "vm_render_viewport_layers_dev")


def _bits(a, b):
    """bit for bit, a NaN for a NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@pytest.mark.parametrize("kind", ["smooth", "rough", "large", "shear", "outside", "nan"])
@pytest.mark.parametrize("with_path", [False, True])
def test_identity_landing_is_the_uniform_statement(kind, with_path):
    """{0, 0, 1, 1, w, h, 1, 1}: ((X + 0.5) * 1 + 0) - 0.5 is X exactly, so the chain from q is sampling_maps' chain"""
    w, h = 45, 23
    rng = np.random.RandomState(41)
    v = warp_ref.field(kind, w, h, rng)
    u = warp_ref.path(w, h, rng) if with_path else None
    vp = Viewport.identity(w, h).astuple()
    (qx, qy), = viewport_ref.sample_points(vp)
    yy, xx = np.mgrid[0:h, 0:w].astype(f32)
    assert np.array_equal(qx, xx) and np.array_equal(qy, yy)
    for geo in (0.0, 0.35, 1.0):
        (m0, m1), = viewport_ref.sample_maps(v, u, geo, vp)
        r0, r1, _, _ = warp_ref.sampling_maps(v, u, geo)
        assert _bits(m0, r0) and _bits(m1, r1), (kind, with_path, geo)


@pytest.mark.parametrize("w,h,ex", SIZES)
def test_identity_bytes_are_the_oracles(oracle, w, h, ex):
    """the cases of tests/test_warp_ref.py::test_statement_maps_give_the_oracles_bytes through the viewport statement"""
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    e0, e1 = morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex)
    rng = np.random.RandomState(41)
    vp = Viewport.identity(w, h).astuple()
    for kind in ("smooth", "rough", "outside"):
        v = warp_ref.field(kind, w, h, rng)
        for with_path in (False, True):
            u = warp_ref.path(w, h, rng) if with_path else None
            uo = u if with_path else np.zeros((h, w, 2), f32)
            for geo in (0.0, 0.35, 1.0):
                out = viewport_ref.render_viewport_bytes(e0, e1, ex, v, u, 0.3, geo, 1, vp)
                ref = oracle.render_halfway(w, h, ex, 0.3, geo, 1, e0.astype(f32), e1.astype(f32), v, uo)
                assert np.array_equal(out, ref), (kind, with_path, geo, int((out != ref).sum()))


@pytest.mark.parametrize("with_path", [False, True])
def test_an_integer_crop_is_the_slice(with_path):
    w, h, ex = 45, 23, 4
    rng = np.random.RandomState(7)
    v = warp_ref.field("smooth", w, h, rng)
    u = warp_ref.path(w, h, rng) if with_path else None
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    e0, e1 = morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex)
    l0, l1 = rgb0.astype(f32) / f32(3), rgb1.astype(f32) / f32(7)
    m0, m1, _, _ = warp_ref.sampling_maps(v, u, 0.35)
    full_b, full_l = warp_ref.render_bytes(e0, e1, ex, m0, m1, 0.3, 1), warp_ref.render_layers(l0, l1, m0, m1, 0.3, 1)
    for x, y, cw, ch in ((0, 0, w, h), (7, 3, 20, 11), (w - 1, h - 1, 1, 1), (13, 0, 5, h)):
        vp = Viewport.crop(x, y, cw, ch).astuple()
        assert np.array_equal(viewport_ref.render_viewport_bytes(e0, e1, ex, v, u, 0.3, 0.35, 1, vp), full_b[y:y + ch, x:x + cw])
        assert _bits(viewport_ref.render_viewport_layers(l0, l1, v, u, 0.3, 0.35, 1, vp), full_l[y:y + ch, x:x + cw])
        got = viewport_ref.render_viewport_layers(l0[..., 0], l1[..., 0], v, u, 0.3, 0.35, 1, vp)
        assert got.shape == (ch, cw) and _bits(got, full_l[y:y + ch, x:x + cw, 0])


def test_half_size_with_2x2_samples_is_the_exact_box():
    """zero field, no path, {0, 0, 2, 2, w / 2, h / 2, 2, 2}: fx is 0.25 / 0.75, q is 2X / 2X + 1, every tap lands on a
    texel, and the result is (uint8)(sum / 4 + 0.5) of each 2 x 2 block of a random canvas, byte for byte"""
    w, h, ex = 46, 22, 3
    rng = np.random.RandomState(3)
    rgb0 = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    rgb1 = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    e0, e1 = morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex)
    v = np.zeros((h, w, 2), f32)
    vp = Viewport.fit(w, h, w // 2, h // 2).supersampled(2)
    assert vp.astuple() == (0.0, 0.0, 2.0, 2.0, w // 2, h // 2, 2, 2)
    pts = viewport_ref.sample_points(vp.astuple())
    assert [(float(qx[0, 1]), float(qy[1, 0])) for qx, qy in pts] == [(2.0, 2.0), (3.0, 2.0), (2.0, 3.0), (3.0, 3.0)]
    got = viewport_ref.render_viewport_bytes(e0, e1, ex, v, None, 0.3, 0.35, 0, vp.astuple())
    s = rgb0.astype(np.int64)
    box = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
    assert np.array_equal(got, (box / 4.0 + 0.5).astype(np.uint8))
    got = viewport_ref.render_viewport_bytes(e0, e1, ex, v, None, 0.3, 0.35, 2, vp.astuple())
    s = rgb1.astype(np.int64)
    box = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
    assert np.array_equal(got, (box / 4.0 + 0.5).astype(np.uint8))


@pytest.mark.parametrize("nx,ny", [(1, 1), (2, 2), (3, 2), (8, 8), (64, 1), (5, 7)])
def test_a_constant_canvas_gives_the_constant(nx, ny):
    """under any viewport and any N, whatever the field: a tap of a constant c <= 255 is c to a few ulp (its four weights
    sum to one to a rounding), the sum of N <= 64 of them is at most 16320 and carries N roundings of at most 2^-10 each,
    so the mean is within 0.1 of c and (uint8)(mean + 0.5) is c.  Where every sample lands on a texel the weights are
    1, 0, 0, 0, c * N is exact and so is its division: then the float layers are the constant bit for bit too."""
    w, h, ex = 19, 11, 5
    c = 213
    rgb = np.full((h, w, 3), c, np.uint8)
    e = np.full((h + 2 * ex, w + 2 * ex, 4), c, np.uint8)
    v = warp_ref.field("smooth", w, h, None)
    for vp in ((0.0, 0.0, 1.0, 1.0, w, h), (3.25, 1.5, 0.4, 0.4, 9, 7), (0.0, 0.0, 2.0, 2.0, 9, 5), (-5.0, -5.0, 1.0, 1.0, 12, 4),
               (-40.0, -30.0, 0.75, 1.5, 5, 3), (100.0, 50.0, 3.0, 3.0, 2, 2)):
        vp = vp + (nx, ny)
        for cf in (0, 1, 2):
            got = viewport_ref.render_viewport_bytes(e, e, ex, v, None, 0.3, 0.35, cf, vp)
            assert got.shape == (vp[5], vp[4], 3) and np.all(got == c), (vp, cf)
    # samples on texels: a zero field, nx x ny field pixels per output pixel: sample (i, j) stands at q = (nx X + i, ny Y + j)
    vp = (0.0, 0.0, float(nx), float(ny), 3, 2, nx, ny)
    for qx, qy in viewport_ref.sample_points(vp):
        assert np.array_equal(qx, np.rint(qx)) and np.array_equal(qy, np.rint(qy))
    zero = np.zeros((h, w, 2), f32)
    for cf in (0, 2):
        lay = viewport_ref.render_viewport_layers(rgb.astype(f32), rgb.astype(f32), zero, None, 0.3, 0.35, cf, vp)
        assert lay.shape == (2, 3, 3) and np.all(lay == f32(c)), (nx, ny, cf)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 64])
def test_the_sample_grid_is_symmetric_about_the_pixel_centre(n):
    """f_i + f_(n - 1 - i) = 1 to a rounding (exactly where the fractions are dyadic), increasing, inside (0, 1); the
    middle one of an odd n is 0.5"""
    f = viewport_ref.sample_fractions(n)
    assert f.dtype == np.float32 and f.shape == (n,)
    assert np.all(f > 0) and np.all(f < 1) and np.all(np.diff(f) > 0)
    assert np.abs((f + f[::-1]) - f32(1)).max() <= 2.0 ** -23
    if n & (n - 1) == 0:
        assert np.array_equal(f + f[::-1], np.ones(n, f32))
    if n % 2:
        assert f[n // 2] == f32(0.5)


def test_sample_order_is_i_fastest():
    vp = (0.0, 0.0, 1.0, 1.0, 2, 2, 3, 2)
    pts = viewport_ref.sample_points(vp)
    assert len(pts) == 6
    xs = [float(qx[0, 0]) for qx, _ in pts]
    ys = [float(qy[0, 0]) for _, qy in pts]
    assert xs[0] < xs[1] < xs[2] and xs[:3] == xs[3:] and ys[0] == ys[1] == ys[2] < ys[3] == ys[4] == ys[5]


def test_constructors():
    assert Viewport.identity(640, 360).astuple() == (0.0, 0.0, 1.0, 1.0, 640, 360, 1, 1)
    assert Viewport.crop(7, 3, 20, 11).astuple() == (7, 3, 1.0, 1.0, 20, 11, 1, 1)
    assert Viewport.fit(1920, 1080, 960, 540).astuple() == (0.0, 0.0, 2.0, 2.0, 960, 540, 1, 1)
    assert Viewport.fit(1920, 1080, 3840, 2160).supersampled(2).astuple() == (0.0, 0.0, 0.5, 0.5, 3840, 2160, 2, 2)
    # a 2.5x zoom of 480 x 270 output pixels covers 192 x 108 field pixels around its centre
    z = Viewport.zoom(100.0, 60.0, 2.5, 480, 270)
    assert z.step_x == z.step_y == 0.4 and abs(z.x0 - 4.0) < 1e-9 and abs(z.y0 - 6.0) < 1e-9
    assert Viewport.overscan(640, 360, 16).astuple() == (-16.0, -16.0, 1.0, 1.0, 672, 392, 1, 1)
    assert Viewport.identity(4, 4).supersampled(3, 2).astuple()[6:] == (3, 2)
    assert Viewport.identity(4, 4) == Viewport.crop(0.0, 0.0, 4, 4) and Viewport.identity(4, 4) != Viewport.identity(4, 5)
    s = Viewport.zoom(100.0, 60.0, 2.5, 480, 270).supersampled(2).struct()
    assert (s.step_x, s.out_w, s.out_h, s.nx, s.ny) == (f32(0.4), 480, 270, 2, 2)


def test_the_validator_refuses_what_the_abi_refuses():
    """every VM_E_INVALID case of a viewport (tests/test_gpu_viewport.py sends the same list to the library), and the
    edges that are legal"""
    for vp in viewport_ref.INVALID_VIEWPORTS:
        with pytest.raises(ValueError):
            Viewport(*vp).validate()
    for vp in viewport_ref.EDGE_VIEWPORTS:
        assert Viewport(*vp).validate().astuple() == vp


def test_the_struct_layout_matches_the_header(tmp_path):
    """vm_viewport as gcc lays it out: 32 bytes, the offsets of the ctypes binding"""
    prog = tmp_path / "vp.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmorph.h"\nint main(void){printf("%zu", sizeof(vm_viewport));'
                    + "".join('printf(" %%zu", offsetof(vm_viewport, %s));' % n for n, _ in capi.ViewportStruct._fields_)
                    + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "vp"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert got[0] == C.sizeof(capi.ViewportStruct)
    assert got[1:] == [getattr(capi.ViewportStruct, n).offset for n, _ in capi.ViewportStruct._fields_]
    assert [n for n, _ in capi.ViewportStruct._fields_] == list(Viewport.__slots__)


def test_the_entry_points_exist(vmlib):
    for n in NAMES:
        assert n in capi.SYMBOLS, n
        assert hasattr(vmlib, n), "libvmorph_hip.so does not export %s" % n
    for n in ("render_viewport", "render_viewport_dev", "render_viewport_layers", "render_viewport_layers_dev"):
        assert callable(getattr(morph.Frame, n))


def test_a_null_frame_is_refused(vmlib):
    buf = C.create_string_buffer(64)
    ms = C.c_float(0)
    vp = Viewport.identity(2, 2).struct()
    assert vmlib.vm_render_viewport(None, C.byref(vp), 0.5, 0.5, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_render_viewport:" in vmlib.vm_last_error()
    assert vmlib.vm_render_viewport_dev(None, C.byref(vp), 0.5, 0.5, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_render_viewport_dev:" in vmlib.vm_last_error()
    assert vmlib.vm_render_viewport_layers(None, C.byref(vp), 0.5, 0.5, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_render_viewport_layers:" in vmlib.vm_last_error()
    assert vmlib.vm_render_viewport_layers_dev(None, C.byref(vp), 0.5, 0.5, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_render_viewport_layers_dev:" in vmlib.vm_last_error()
