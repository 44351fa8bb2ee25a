"""tests/vshutter_ref.py, the statement of a viewport over a shutter, pinned without a GPU to the statements it composes:
with one time sample it is viewport_ref, at the identity viewport it is shutter_ref and transit_shutter_ref, and under
the schedule (0, 1) with the linear ease the scheduled family is the uniform one -- maps, bytes and layers bit for bit."""
import numpy as np
import pytest

import chain_ref
import shutter_ref
from render_cases import field as _field, same_bits as _same
import transit_ref
import transit_shutter_ref as TS
import viewport_ref
import vshutter_ref as VS
from videomorphing_amd import transition
from videomorphing_amd.viewport import Viewport

f32 = np.float32
SHAPES = [(33, 7, 3), (5, 3, 2)]
KINDS = ["smooth", "large", "outside", "nan"]
SHUTTERS = ((0.3, 0.7), (0.0, 1.0), (-0.2, 0.2), (0.7, 1.3), (0.7, 0.3))
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)
kinds = pytest.mark.parametrize("kind", KINDS)
cases = pytest.mark.parametrize("with_path", [False, True])


def _canvases(w, h, ex):
    rng = np.random.RandomState(5)
    return [rng.randint(0, 256, (h + 2 * ex, w + 2 * ex, 4)).astype(np.uint8) for _ in range(2)]


def _layers(w, h, c, seed):
    rng = np.random.RandomState(seed)
    a = (rng.randn(h, w, c) * 10.0 ** rng.randint(-6, 6, (h, w, c))).astype(f32)
    return a[..., 0] if c == 1 else a


def _same_maps(got, want):
    return len(got) == len(want) and all(len(g) == len(w) and all(_same(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))


def _viewports(w, h):
    return [Viewport(1.25, 0.5, 0.4, 0.4, 12, 7, 3, 2), Viewport(0.5, 0.5, 1.0, 1.0, w, h, 2, 2),
            Viewport(0.0, 0.0, 2.0, 2.0, (w + 1) // 2, (h + 1) // 2, 1, 1), Viewport(w / 3.0, h / 2.0, 0.7, 0.7, 1, 1, 8, 8)]


@shapes
@kinds
@cases
def test_one_time_sample_is_the_viewport_statement(w, h, ex, kind, with_path):
    v, u = _field(w, h, kind, with_path)
    e0, e1 = _canvases(w, h, ex)
    l0, l1 = _layers(w, h, 3, 1), _layers(w, h, 3, 2)
    for at, vp in enumerate(_viewports(w, h)):
        for g in ((0.0, 0.3, 1.0) if at == 0 else (0.3,)):
            maps = VS.uniform_maps(v, u, g, g, 1, vp.astuple())
            want = viewport_ref.sample_maps(v, u, g, vp.astuple())
            assert _same_maps(maps, want), (vp, g)
            ok = chain_ref.founded(maps)
            for cf in (0, 1, 2):
                a = VS.bytes_on_maps(e0, e1, ex, maps, cf, 0.3)
                b = viewport_ref.render_viewport_bytes(e0, e1, ex, v, u, 0.3, g, cf, vp.astuple(), want)
                assert np.array_equal(a[ok], b[ok])
                assert _same(VS.layers_on_maps(l0, l1, maps, cf, 0.3), viewport_ref.layers_on_maps(l0, l1, want, 0.3, cf))


@shapes
@kinds
@cases
def test_the_identity_viewport_is_the_shutter_statements(w, h, ex, kind, with_path):
    v, u = _field(w, h, kind, with_path)
    e0, e1 = _canvases(w, h, ex)
    ident = Viewport.identity(w, h).astuple()
    sg, sc = transition.wipe(w, h), transition.radial(w, h)
    for c in (1, 3):
        l0, l1 = _layers(w, h, c, 1), _layers(w, h, c, 2)
        for n, (o, cl) in zip((1, 2, 5, 3, 2), SHUTTERS):
            maps = VS.uniform_maps(v, u, o, cl, n, ident)
            want = shutter_ref.sample_maps(v, u, o, cl, n)
            assert _same_maps(maps, want), (n, o, cl)
            ok = chain_ref.founded(maps)
            a = VS.render_viewport_shutter_bytes(e0, e1, ex, v, u, 0.3, o, cl, n, 1, ident)
            assert np.array_equal(a[ok], shutter_ref.render_shutter_bytes(e0, e1, ex, v, u, 0.3, o, cl, n, 1)[ok])
            assert _same(VS.layers_on_maps(l0, l1, maps, 1, 0.3), shutter_ref.layers_on_maps(l0, l1, want, 0.3, 1))
            for ease in (0, 1):
                maps = VS.scheduled_maps(v, u, sg, sc, o, cl, n, 0.45, ease, ident)
                want = TS.sample_maps(v, u, sg, sc, o, cl, n, 0.45, ease)
                assert _same_maps(maps, want), (n, o, cl, ease)
                ok = chain_ref.founded(maps)
                a = VS.bytes_on_maps(e0, e1, ex, maps, 1)
                assert np.array_equal(a[ok], chain_ref.bytes_of(TS.canvas_mean(e0, e1, ex, want, 1))[ok])
                assert _same(VS.layers_on_maps(l0, l1, maps, 1), TS.layers_on_maps(l0, l1, want, 1))


@shapes
@kinds
@cases
def test_the_uniform_schedule_is_the_uniform_family(w, h, ex, kind, with_path):
    """schedule (0, 1) on both planes, linear ease: the maps of the uniform family, and k == t_color in [0, 1] exactly
    wherever the chain's last position is finite (k is tapped there)"""
    v, u = _field(w, h, kind, with_path)
    e0, e1 = _canvases(w, h, ex)
    l0, l1 = _layers(w, h, 2, 1), _layers(w, h, 2, 2)
    uni = transit_ref.uniform_schedule(w, h)
    for at, vp in enumerate(_viewports(w, h)[:3]):
        for n, (o, cl) in zip((1, 2, 5, 3, 2), SHUTTERS):
            for tc in ((0.0, 0.3, 1.0) if at == 0 and n == 2 else (0.3,)):
                got = VS.scheduled_maps(v, u, uni, None, o, cl, n, tc, 0, vp.astuple())
                want = VS.uniform_maps(v, u, o, cl, n, vp.astuple())
                assert _same_maps([m[:2] for m in got], want), (vp, n, o, cl)
                for m0, m1, k in got:
                    there = np.isfinite(m0).all(-1) & np.isfinite(m1).all(-1)
                    assert kind == "nan" or there.all()
                    assert np.array_equal(k[there], np.full(int(there.sum()), f32(tc)))
                ok = chain_ref.founded(want)
                for cf in (0, 1, 2):
                    assert np.array_equal(VS.bytes_on_maps(e0, e1, ex, got, cf)[ok], VS.bytes_on_maps(e0, e1, ex, want, cf, tc)[ok])
                    assert _same(VS.layers_on_maps(l0, l1, got, cf), VS.layers_on_maps(l0, l1, want, cf, tc))


def test_the_loop_order_is_time_outside_and_sub_samples_inside():
    """T * N maps, the N of one time first: the sum in float32 depends on the order"""
    w, h = 33, 7
    v, u = _field(w, h, "smooth", True)
    vp = Viewport(1.25, 0.5, 0.4, 0.4, 6, 4, 3, 2).astuple()
    maps = VS.uniform_maps(v, u, 0.2, 0.8, 4, vp)
    assert len(maps) == 24
    times = shutter_ref.sample_times(0.2, 0.8, 4)
    for tau in range(4):
        assert _same_maps(maps[6 * tau:6 * tau + 6], viewport_ref.sample_maps(v, u, times[tau], vp))
    with pytest.raises(AssertionError):
        VS.uniform_maps(v, u, 0.2, 0.8, 5, (0.0, 0.0, 1.0, 1.0, 2, 2, 8, 8))       # 320 chains: above the cap
    assert len(VS.uniform_maps(v, u, 0.2, 0.8, 4, (0.0, 0.0, 1.0, 1.0, 2, 2, 8, 8))) == 256
