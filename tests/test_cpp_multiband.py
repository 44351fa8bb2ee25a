"""The C++ facade of the multiband calls (include/vmorph/render.hpp: vmorph::Bands; examples/multiband.cpp) builds with
plain g++ against the C-ABI, and on a GPU writes the files the Python facade's arrays give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph, transition
from videomorphing_amd.multiband import Bands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def multiband_exe(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppmb") / "multiband")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "multiband.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_multiband_driver_builds(multiband_exe):
    assert os.path.exists(multiband_exe)
    r = subprocess.run([multiband_exe], capture_output=True, text=True)      # no arguments: usage, nothing touched
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
def test_multiband_driver_matches_python_facade(multiband_exe, gpu_ctx, tmp_path):
    w, h, seed, margin = 150, 97, 5, 12
    prefix = str(tmp_path / "m")
    r = subprocess.run([multiband_exe, str(w), str(h), str(seed), str(margin), prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rgb0, rgb1, v = _inputs(w, h, seed)
    fr = morph.Frame(gpu_ctx, w, h, margin)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(v=v)
    fr.upload_schedule(None, transition.wipe(w, h, lead=1.0, duration=0.0))
    levels = Bands.for_size(w, h).levels
    assert levels == 5
    pictures = {
        "_dissolve_plain.ppm": fr.render_halfway(0.4, 0.4, 1),
        "_dissolve_bands.ppm": fr.render_multiband(Bands.sharpen(levels, 8.0), 0.4, 0.4),
        "_wipe_plain.ppm": fr.render_transition(0.5),
        "_wipe_bands.ppm": fr.render_multiband_transition(Bands.linear(levels), 0.5),
    }
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    for name, want in pictures.items():
        raw = open(prefix + name, "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * w * h, name
        assert raw[len(head):] == want.tobytes(), name

    def differing(a, b):
        return int((a != b).any(axis=-1).sum())

    d_dissolve = differing(pictures["_dissolve_plain.ppm"], pictures["_dissolve_bands.ppm"])
    d_wipe = differing(pictures["_wipe_plain.ppm"], pictures["_wipe_bands.ppm"])
    assert d_dissolve > 0 and d_wipe > 0
    assert r.stdout.strip() == ("%dx%d in %d levels: at t = 0.4 the sharpened dissolve differs from the plain one in %d of %d pixels, "
                                "the multiband wipe at t = 0.5 from the hard one in %d" % (w, h, levels, d_dissolve, w * h, d_wipe))
    fr.close()
