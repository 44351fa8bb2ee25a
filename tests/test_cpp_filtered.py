"""The C++ facade of the filtered viewport calls (include/vmorph/render.hpp: vmorph::Filter; examples/zoom_filtered.cpp)
builds with plain g++ against the C-ABI, and on a GPU writes the files the Python facade's arrays give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph
from videomorphing_amd.viewport import Viewport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def zoom_exe(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppf") / "zoom_filtered")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "zoom_filtered.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_zoom_driver_builds(zoom_exe):
    assert os.path.exists(zoom_exe)
    r = subprocess.run([zoom_exe], capture_output=True, text=True)      # no arguments: usage, nothing touched
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
    matte0 = (tri(x + y + seed, 8) >= 4).astype(f32)
    matte1 = (tri(x + y + seed - 3, 8) >= 4).astype(f32)
    return rgb0, rgb1, v, matte0, matte1


@pytest.mark.gpu
def test_zoom_driver_matches_python_facade(zoom_exe, gpu_ctx, tmp_path):
    w, h, seed, margin = 150, 97, 5, 12
    prefix = str(tmp_path / "z")
    r = subprocess.run([zoom_exe, str(w), str(h), str(seed), str(margin), prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rgb0, rgb1, v, matte0, matte1 = _inputs(w, h, seed)
    fr = morph.Frame(gpu_ctx, w, h, margin)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(v=v)
    fr.upload_layers(matte0, matte1)
    zoom = Viewport.zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 4.0, w, h)
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pictures = {}
    for name, filt in (("_bilinear.ppm", capi.FILTER_BILINEAR), ("_catmull_rom.ppm", capi.FILTER_CATMULL_ROM),
                       ("_mitchell.ppm", capi.FILTER_MITCHELL)):
        raw = open(prefix + name, "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * w * h, name
        pictures[name] = fr.render_viewport_filtered(zoom, filt, 0.5, 0.5, 1)
        assert raw[len(head):] == pictures[name].tobytes(), name
    assert np.array_equal(pictures["_bilinear.ppm"], fr.render_viewport(zoom, 0.5, 0.5, 1))
    assert not np.array_equal(pictures["_bilinear.ppm"], pictures["_catmull_rom.ppm"])
    assert not np.array_equal(pictures["_mitchell.ppm"], pictures["_catmull_rom.ppm"])
    matte = fr.render_viewport_filtered_layers(zoom, capi.FILTER_CATMULL_ROM, 0.5, 0.5, 1)
    outside = int(((matte < 0) | (matte > 1)).sum())
    assert outside > 0                                                 # the stripes ring: the call does not clamp
    grey = (np.clip(matte, f32(0), f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)
    head = ("P5\n%d %d\n255\n" % (w, h)).encode()
    raw = open(prefix + "_matte.pgm", "rb").read()
    assert raw.startswith(head) and raw[len(head):] == grey.tobytes()
    assert r.stdout.strip() == ("%dx%d at t = 0.5: a 4x zoom from (%g, %g) in bilinear, Catmull-Rom and Mitchell; the matte through "
                                "Catmull-Rom leaves [0, 1] in %d of %d pixels" % (w, h, f32(zoom.x0), f32(zoom.y0), outside, w * h))
    fr.close()
