"""The C++ facade of the error view (include/vmorph/pyramid.hpp, morph.hpp; examples/error_image.cpp) builds with plain
g++ against the C-ABI, and on a GPU prints the totals and writes the image the Python facade gives for the same pair."""
import os
import re
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def error_image(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppe") / "error_image")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "error_image.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def test_error_driver_builds(error_image):
    assert os.path.exists(error_image)
    r = subprocess.run([error_image], capture_output=True, text=True)      # no arguments: usage, nothing touched
    assert r.returncode == 2 and "usage" in r.stderr


def _pair(w, h, seed):
    """the driver's synthetic pair: integer triangle waves, img1 = img0 moved by (2, 1)"""
    def tri(a, p):
        return np.abs(a % (2 * p) - p)

    def pattern(x, y):
        return (tri(3 * x + 2 * y + seed, 37) + tri(5 * y - x + 7 * seed, 53)).astype(np.float32) * (np.float32(255.0) / np.float32(90.0))

    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return pattern(x, y), pattern(x - 2, y - 1)


@pytest.mark.gpu
def test_error_driver_matches_python_facade(error_image, gpu_ctx, tmp_path):
    w, h, seed, what, gain = 150, 97, 5, capi.ERR_SSIM, 150.0
    out = tmp_path / "e.ppm"
    r = subprocess.run([error_image, str(w), str(h), str(seed), str(out), "6", "exact", str(what), str(gain)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = re.findall(r"^level (\d+) (\d+)x(\d+) ssim (\S+) tps (\S+) ui (\S+) temp (\S+) all (\S+)$", r.stdout, re.M)
    raw = open(str(out), "rb").read()
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h * 3
    img_cpp = np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)

    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    i0, i1 = _pair(w, h, seed)
    prm = morph.Parameters()
    prm.max_iter, prm.max_iter_drop_factor, prm.start_res = 6, 1.0, 32
    pyr = morph.Pyramid(gpu_ctx)
    pyr.build(i0, i1, 32)
    t = morph.MatchingThread(prm, pyr, keep_state=True)
    t.start()
    t.wait()
    assert len(rows) == pyr.size() - 2 == len(t.energies)
    for el, lw, lh, *e in rows:
        want = t.energies[int(el)]
        assert (int(lw), int(lh)) == (pyr[int(el)].width, pyr[int(el)].height)
        assert [float(x) for x in e] == [want[k] for k in capi.ERR_NAMES]      # %.17g round-trips a double
    img_py = pyr[1].error_image(w, h, what, gain)
    assert np.array_equal(img_cpp, img_py)
    assert len(np.unique(img_py.reshape(-1, 3), axis=0)) > 1                   # a picture, not one colour
