"""The C++ facade of the shutter calls under a transition schedule (include/vmorph/render.hpp;
examples/transition_blur.cpp) builds with plain g++ against the C-ABI, and on a GPU writes the files the Python facade's
arrays give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def transition_blur_exe(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppts") / "transition_blur")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "transition_blur.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_transition_blur_driver_builds(transition_blur_exe):
    assert os.path.exists(transition_blur_exe)
    r = subprocess.run([transition_blur_exe], capture_output=True, text=True)      # no arguments: usage, nothing touched
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
    m0 = tri(x + y + seed, 16).astype(f32) * f32(0.0625)
    m1 = tri(x - y + seed, 16).astype(f32) * f32(0.0625)
    t0 = f32(0.6) * (x.astype(f32) / f32(max(w - 1, 1)))
    wipe = np.stack([t0, t0 + f32(0.4)], -1)
    assert wipe.dtype == np.float32
    return rgb0, rgb1, v, m0, m1, wipe


@pytest.mark.gpu
def test_transition_blur_driver_matches_python_facade(transition_blur_exe, gpu_ctx, tmp_path):
    w, h, seed = 150, 97, 5
    prefix = str(tmp_path / "t")
    r = subprocess.run([transition_blur_exe, str(w), str(h), str(seed), prefix], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rgb0, rgb1, v, m0, m1, wipe = _inputs(w, h, seed)
    fr = morph.Frame(gpu_ctx, w, h, 0)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(v=v)
    fr.upload_layers(m0, m1)
    fr.upload_schedule(wipe, wipe)

    def body(name, magic, size):
        head = ("%s\n%d %d\n255\n" % (magic, w, h)).encode()
        raw = open(prefix + name, "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + size, name
        return raw[len(head):]

    sharp = fr.render_transition(0.5)
    assert body("_sharp.ppm", "P6", 3 * w * h) == sharp.tobytes()
    blur = fr.render_transition_shutter(f32(0.45), f32(0.55), 16, 0.5)
    assert body("_blur.ppm", "P6", 3 * w * h) == blur.tobytes()
    matte = fr.render_transition_shutter_layers(f32(0.45), f32(0.55), 16, 0.5)
    assert matte.shape == (h, w) and matte.min() >= 0 and matte.max() <= 1
    assert body("_matte.pgm", "P5", w * h) == (matte * f32(255) + f32(0.5)).astype(np.uint8).tobytes()
    moved = int((sharp != blur).sum())
    assert moved > 0
    assert r.stdout.strip() == ("%dx%d: a wipe at t = 0.5 sharp and over a shutter 0.45 .. 0.55 of 16 samples; %d of %d bytes differ"
                                % (w, h, moved, 3 * w * h))
    fr.close()
