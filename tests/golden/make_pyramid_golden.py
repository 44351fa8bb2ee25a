"""Generates tests/golden/pyramid_ref.npz and pyramid_edges_ref.npz: luma pyramids computed by the REFERENCE's own
resampling library (oracle/_ref/libresample_ref.so, built by `make -C oracle ref` from
/root/reference/include/resample where it lies) for small synthetic RGB frames.
Run in the build container (the reference is not available on the GPU box):
    python tests/golden/make_pyramid_golden.py
The fixtures hold data only: input frames (uint8) and the expected level lumas; the edge cases (thin, tiny
and odd frames, tests/pyramid_cases.py) are generated from seeds, so their file holds the lumas alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyramid_cases  # noqa: E402
from videomorphing_amd import synth  # noqa: E402

subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libresample_ref.so"))
lib.ref_luma_pyramid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]


def run(rgb, nlevels):
    h, w = rgb.shape[:2]
    data = np.ascontiguousarray(rgb, dtype=np.float32)
    sizes, ww, hh = [], w, h
    for _ in range(nlevels):
        sizes.append((ww, hh))
        ww, hh = (ww + 1) // 2, (hh + 1) // 2
    out = np.zeros(sum(a * b for a, b in sizes), dtype=np.float32)
    lib.ref_luma_pyramid(data.ctypes.data, w, h, nlevels, out.ctypes.data)
    return out


cases = {}
for name, (w, h, nl, frame) in {"a": (75, 52, 3, 0), "b": (64, 48, 3, 1), "c": (33, 21, 2, 2)}.items():
    rgb0, rgb1 = synth.make_rgb_pair(w, h, frame=frame)
    rng = np.random.RandomState(7 + frame)           # some hard edges and saturated pixels too
    rgb1 = rgb1.copy()
    rgb1[h // 3:h // 2, w // 4:w // 2] = rng.randint(0, 256, size=(h // 2 - h // 3, w // 2 - w // 4, 3))
    for k, rgb in (("0", rgb0), ("1", rgb1)):
        cases["%s%s_rgb" % (name, k)] = rgb
        cases["%s%s_nlevels" % (name, k)] = np.int32(nl)
        cases["%s%s_luma" % (name, k)] = run(rgb, nl)
np.savez_compressed(os.path.join(HERE, "pyramid_ref.npz"), **cases)
print("wrote", os.path.join(HERE, "pyramid_ref.npz"), {k: v.shape for k, v in cases.items() if k.endswith("luma")})

edges = {name: run(pyramid_cases.edge_rgb(name), nl) for name, (_, _, nl, _) in pyramid_cases.LUMA_EDGES.items()}
np.savez_compressed(os.path.join(HERE, "pyramid_edges_ref.npz"), **edges)
print("wrote", os.path.join(HERE, "pyramid_edges_ref.npz"), {k: v.shape for k, v in edges.items()})
