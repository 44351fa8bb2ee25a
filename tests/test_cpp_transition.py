"""The C++ facade of transition control (include/vmorph/render.hpp; examples/transition.cpp) builds with plain g++
against the C-ABI, and on a GPU writes the files the Python facade's arrays give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def transition_exe(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppt") / "transition")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "transition.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_transition_driver_builds(transition_exe):
    assert os.path.exists(transition_exe)
    r = subprocess.run([transition_exe], capture_output=True, text=True)      # no arguments: usage, nothing touched
    assert r.returncode == 2 and "usage" in r.stderr


def _inputs(w, h, seed):
    """the driver's inputs: integer triangle waves, and the wipe in the driver's float32 expressions"""
    def tri(a, p):
        return np.abs(a % (2 * p) - p)

    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    c = np.arange(3).reshape(1, 1, 3)
    rgb0 = (4 * tri(3 * x[..., None] + 2 * y[..., None] + seed + 11 * c, 31)).astype(np.uint8)
    rgb1 = (4 * tri(3 * (x[..., None] - 4) + 2 * (y[..., None] - 2) + seed + 11 * c, 31)).astype(np.uint8)
    v = np.stack([(tri(2 * x + y + seed, 29) - 14).astype(f32) * f32(0.25),
                  (tri(x + 3 * y + 5 * seed, 41) - 20).astype(f32) * f32(0.125)], -1)
    t0 = f32(0.5) * (x.astype(f32) / f32(w - 1))
    return rgb0, rgb1, v, np.stack([t0, t0 + f32(0.5)], -1)


@pytest.mark.gpu
def test_transition_driver_matches_python_facade(transition_exe, gpu_ctx, tmp_path):
    w, h, seed = 150, 97, 5
    prefix = str(tmp_path / "t")
    r = subprocess.run([transition_exe, str(w), str(h), str(seed), prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rgb0, rgb1, v, wipe = _inputs(w, h, seed)
    assert wipe.dtype == f32
    fr = morph.Frame(gpu_ctx, w, h, 0)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(v=v)
    fr.upload_schedule(wipe, wipe)
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    pictures, worst = [], f32(0)
    for k in range(3):
        t = 0.25 * (k + 1)
        raw = open("%s_%d.ppm" % (prefix, k), "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * w * h
        want = fr.render_transition(t, capi.EASE_SMOOTH, 1)
        assert raw[len(head):] == want.tobytes(), k
        pictures.append(want)
        worst = max(worst, fr.transition_maps(t, capi.EASE_SMOOTH)[2].max())
    # a wipe: at t = 0.75 the left half has arrived at the end of the morph, at t = 0.25 the right half has not left its
    # beginning (8 columns: more than the field's 3.5 px and the taps' reach)
    assert np.array_equal(pictures[2][:, :w // 2 - 8], fr.render_halfway(1.0, 1.0, 1)[:, :w // 2 - 8])
    assert np.array_equal(pictures[0][:, w // 2 + 8:], fr.render_halfway(0.0, 0.0, 1)[:, w // 2 + 8:])
    assert not np.array_equal(pictures[0], pictures[2])
    assert r.stdout.strip() == "%dx%d: a wipe at t = 0.25, 0.5, 0.75; the last round moved %g px at most" % (w, h, worst)
    fr.close()
