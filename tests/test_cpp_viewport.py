"""The C++ facade of the viewport calls (include/vmorph/render.hpp; examples/viewport.cpp) builds with plain g++ against the
C-ABI, and on a GPU writes the files the Python facade's arrays give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph
from videomorphing_amd.viewport import Viewport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def viewport_exe(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppv") / "viewport")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "viewport.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_viewport_driver_builds(viewport_exe):
    assert os.path.exists(viewport_exe)
    r = subprocess.run([viewport_exe], capture_output=True, text=True)      # no arguments: usage, nothing touched
    assert r.returncode == 2 and "usage" in r.stderr


def _inputs(w, h, seed):
    """the driver's inputs: integer triangle waves in the driver's float32 expressions"""
    def tri(a, p):
        return np.abs(a % (2 * p) - p)

    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    c = np.arange(3).reshape(1, 1, 3)
    rgb0 = (4 * tri(3 * x[..., None] + 2 * y[..., None] + seed + 11 * c, 31)).astype(np.uint8)
    rgb1 = (4 * tri(3 * (x[..., None] - 4) + 2 * (y[..., None] - 2) + seed + 11 * c, 31)).astype(np.uint8)
    v = np.stack([(tri(2 * x + y + seed, 29) - 14).astype(f32),
                  (tri(x + 3 * y + 5 * seed, 41) - 20).astype(f32) * f32(0.5)], -1)
    return rgb0, rgb1, v


@pytest.mark.gpu
def test_viewport_driver_matches_python_facade(viewport_exe, gpu_ctx, tmp_path):
    w, h, seed, margin = 150, 97, 5, 12
    prefix = str(tmp_path / "v")
    r = subprocess.run([viewport_exe, str(w), str(h), str(seed), str(margin), prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rgb0, rgb1, v = _inputs(w, h, seed)
    fr = morph.Frame(gpu_ctx, w, h, margin)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(v=v)
    zoom = Viewport.zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 2.5, w // 2, h // 2)
    vps = {"_native.ppm": Viewport.identity(w, h), "_zoom.ppm": zoom,
           "_proxy.ppm": Viewport.fit(w, h, w // 2, h // 2).supersampled(2), "_overscan.ppm": Viewport.overscan(w, h, margin)}
    for name, vp in vps.items():
        head = ("P6\n%d %d\n255\n" % (vp.out_w, vp.out_h)).encode()
        raw = open(prefix + name, "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * vp.out_w * vp.out_h, name
        assert raw[len(head):] == fr.render_viewport(vp, 0.5, 0.5, 1).tobytes(), name
    assert np.array_equal(fr.render_viewport(vps["_native.ppm"], 0.5, 0.5, 1), fr.render_halfway(0.5, 0.5, 1))
    assert r.stdout.strip() == ("%dx%d at t = 0.5: native, a 2.5x zoom of %dx%d from (%g, %g), a %dx%d proxy of 2x2 samples, "
                                "%dx%d with %d px of overscan" % (w, h, w // 2, h // 2, f32(zoom.x0), f32(zoom.y0), w // 2, h // 2,
                                                                   w + 2 * margin, h + 2 * margin, margin))
    fr.close()
