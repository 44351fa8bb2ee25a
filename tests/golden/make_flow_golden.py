"""Generates tests/golden/flow_ref.npz and flow_edges_ref.npz: optical-flow fields scaled by the REFERENCE's own
resampling library (oracle/_ref/libresample_ref.so, `make -C oracle ref`) in the call order of
the flow half of Pyramid::build (pyramid.cu:284-321, 375-404).  Run in the build container:
    python tests/golden/make_flow_golden.py
The fixtures hold data only: input flows and the expected scaled flows; the edge cases (enlargement, 3 : 1,
odd -> odd, flows at and beyond the +-50 px range, an axis-order tie; tests/pyramid_cases.py) are generated
from seeds, so their file holds the scaled flows alone."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyramid_cases  # noqa: E402
subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libresample_ref.so"))
lib.ref_flow_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]


def _edge(name):
    w, h, wo, ho, _, _ = pyramid_cases.FLOW_EDGES[name]
    out = np.zeros((ho, wo, 2), dtype=np.float32)
    lib.ref_flow_scale(np.ascontiguousarray(pyramid_cases.edge_flow(name)).ctypes.data, w, h, wo, ho, out.ctypes.data)
    return out


if len(sys.argv) == 4 and sys.argv[1] == "--edge":        # one edge case, for the loop below
    np.save(sys.argv[3], _edge(sys.argv[2]))
    sys.exit(0)

# one fresh process per edge case: run one after the other in a single process, the library crashes after the
# 3 : 1 case (each case on its own runs clean and equals the oracle)
edges = {}
with tempfile.TemporaryDirectory() as tmp:
    for name in pyramid_cases.FLOW_EDGES:
        path = os.path.join(tmp, name + ".npy")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--edge", name, path], stdout=subprocess.DEVNULL)
        edges[name] = np.load(path)
np.savez_compressed(os.path.join(HERE, "flow_edges_ref.npz"), **edges)
print({k: v.shape for k, v in edges.items()})

cases = {}
rng = np.random.RandomState(11)
for name, (w, h, wo, ho) in {"same": (40, 28, 40, 28), "half": (40, 28, 20, 14), "odd": (33, 21, 17, 11), "wide": (48, 20, 24, 10)}.items():
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    flow = np.stack([3.0 * np.sin(x / 7.0) + 0.05 * y - 1.5, -2.0 * np.cos(y / 5.0) + 0.02 * x], axis=-1).astype(np.float32)
    flow += rng.randn(h, w, 2).astype(np.float32) * 0.3
    flow[2, 3] = (60.0, -70.0)                 # beyond the [-50, 50] range the reference clamps to
    out = np.zeros((ho, wo, 2), dtype=np.float32)
    lib.ref_flow_scale(np.ascontiguousarray(flow).ctypes.data, w, h, wo, ho, out.ctypes.data)
    cases[name + "_in"] = flow
    cases[name + "_out"] = out
np.savez_compressed(os.path.join(HERE, "flow_ref.npz"), **cases)
print({k: v.shape for k, v in cases.items()})
