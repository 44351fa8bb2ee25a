"""The C++ facade of the carry calls (include/vmorph/render.hpp; examples/carry_points.cpp) builds with plain g++ against
the C-ABI, and on a GPU writes the files the Python facade's arrays give for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def carry_points(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppc") / "carry_points")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "carry_points.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_carry_driver_builds(carry_points):
    assert os.path.exists(carry_points)
    r = subprocess.run([carry_points], capture_output=True, text=True)      # no arguments: usage, nothing touched
    assert r.returncode == 2 and "usage" in r.stderr


def _inputs(w, h, seed):
    """the driver's inputs: integer triangle waves"""
    def tri(a, p):
        return np.abs(a % (2 * p) - p)

    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    c = np.arange(3).reshape(1, 1, 3)
    rgb0 = (4 * tri(3 * x[..., None] + 2 * y[..., None] + seed + 11 * c, 31)).astype(np.uint8)
    rgb1 = (4 * tri(3 * (x[..., None] - 4) + 2 * (y[..., None] - 2) + seed + 11 * c, 31)).astype(np.uint8)
    v = np.stack([(tri(2 * x + y + seed, 29) - 14).astype(f32) * f32(0.25),
                  (tri(x + 3 * y + 5 * seed, 41) - 20).astype(f32) * f32(0.125)], -1)
    return rgb0, rgb1, v


@pytest.mark.gpu
def test_carry_driver_matches_python_facade(carry_points, gpu_ctx, tmp_path):
    w, h, seed = 150, 97, 5
    prefix = str(tmp_path / "c")
    r = subprocess.run([carry_points, str(w), str(h), str(seed), prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rgb0, rgb1, v = _inputs(w, h, seed)
    fr = morph.Frame(gpu_ctx, w, h, 0)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(v=v)
    ring = np.fromfile(prefix + "_ring_start.f32", f32).reshape(24, 2)
    centre, radius = f32([(w - 1) / 2, (h - 1) / 2]), 0.25 * min(w, h)
    assert np.allclose(np.hypot(*(ring - centre).T), radius, atol=1e-3) and len(np.unique(ring, axis=0)) == 24       # a ring
    out, _, _, pos1, _, _ = fr.carry_points(ring, 0.0, [0.0, 0.25, 0.5, 0.75, 1.0])
    assert open(prefix + "_ring.f32", "rb").read() == out.tobytes()
    assert not np.array_equal(out[0], out[4])                           # the markers move
    mv = fr.motion_maps(0.5, [1.0])[0][0]
    yy, xx = np.mgrid[0:h, 0:w].astype(f32)
    mv = mv - np.stack([xx, yy], -1)
    assert mv.dtype == f32 and open(prefix + "_mv.f32", "rb").read() == mv.tobytes()
    cons = [(ring[0, 0], ring[0, 1], pos1[0, 0], pos1[0, 1], 1.0), (ring[0, 0], ring[0, 1], pos1[0, 0] + f32(1), pos1[0, 1], 1.0)]
    g01, g10, r01, r10 = fr.constraint_gaps(cons)
    lines = ["constraint %d: 0 -> 1 misses by %.6f px (resid %.3g), 1 -> 0 by %.6f px (resid %.3g)" % (k, g01[k], r01[k], g10[k], r10[k])
             for k in range(2)]
    assert r.stdout.strip().splitlines() == lines
    assert g01[0] == 0 and abs(float(g01[1]) - 1) < 1e-4     # (the second target is one rounded addition away)
    fr.close()
