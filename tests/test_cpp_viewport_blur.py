"""The C++ facade of the viewport calls over a shutter (include/vmorph/render.hpp; examples/viewport_blur.cpp) builds with
plain g++ against the C-ABI, and on a GPU writes the files the Python facade's arrays give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph
from videomorphing_amd.viewport import Viewport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def viewport_blur_exe(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppvb") / "viewport_blur")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "viewport_blur.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_viewport_blur_driver_builds(viewport_blur_exe):
    assert os.path.exists(viewport_blur_exe)
    r = subprocess.run([viewport_blur_exe], capture_output=True, text=True)      # no arguments: usage, nothing touched
    assert r.returncode == 2 and "usage" in r.stderr


def _inputs(w, h, seed):
    """the driver's inputs: integer triangle waves and the wipe in the driver's float32 expressions"""
    def tri(a, p):
        return np.abs(a % (2 * p) - p)

    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    c = np.arange(3).reshape(1, 1, 3)
    rgb0 = (4 * tri(3 * x[..., None] + 2 * y[..., None] + seed + 11 * c, 31)).astype(np.uint8)
    rgb1 = (4 * tri(3 * (x[..., None] - 4) + 2 * (y[..., None] - 2) + seed + 11 * c, 31)).astype(np.uint8)
    v = np.stack([(tri(2 * x + y + seed, 29) - 14).astype(f32),
                  (tri(x + 3 * y + 5 * seed, 41) - 20).astype(f32) * f32(0.5)], -1)
    t0 = f32(0.6) * (x.astype(f32) / f32(w - 1))
    wipe = np.stack([t0, t0 + f32(0.4)], -1)
    assert wipe.dtype == np.float32
    return rgb0, rgb1, v, wipe


@pytest.mark.gpu
def test_viewport_blur_driver_matches_python_facade(viewport_blur_exe, gpu_ctx, tmp_path):
    w, h, seed = 150, 97, 5
    prefix = str(tmp_path / "vb")
    r = subprocess.run([viewport_blur_exe, str(w), str(h), str(seed), prefix], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rgb0, rgb1, v, wipe = _inputs(w, h, seed)
    fr = morph.Frame(gpu_ctx, w, h, 0)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(v=v)
    fr.upload_schedule(wipe, wipe)
    zoom = Viewport.zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 2.5, w // 2, h // 2)
    proxy = Viewport.fit(w, h, w // 2, h // 2).supersampled(2)

    def body(name, vp):
        head = ("P6\n%d %d\n255\n" % (vp.out_w, vp.out_h)).encode()
        raw = open(prefix + name, "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * vp.out_w * vp.out_h, name
        return raw[len(head):]

    blurred = fr.render_viewport_shutter(zoom, 0.5, f32(0.4), f32(0.6), 16)
    assert body("_zoom.ppm", zoom) == blurred.tobytes()
    assert (blurred != fr.render_viewport(zoom, 0.5, 0.5)).any()            # the shutter is no instant
    over = fr.render_viewport_transition_shutter(proxy, f32(0.45), f32(0.55), 16, 0.5)
    assert body("_proxy.ppm", proxy) == over.tobytes()
    still = fr.render_viewport_transition(proxy, 0.5)
    assert body("_still.ppm", proxy) == still.tobytes()
    assert (over != still).any()
    assert r.stdout.strip() == ("%dx%d: a 2.5x zoom of %dx%d from (%g, %g) over a shutter of 16 samples, a %dx%d proxy of 2x2 samples "
                                "of a wipe over one and at t = 0.5" % (w, h, w // 2, h // 2, f32(zoom.x0), f32(zoom.y0), w // 2, h // 2))
    fr.close()
