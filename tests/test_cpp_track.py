"""The C++ facade of the stage-2 point tracker (include/vmorph/track.hpp, examples/track_points.cpp) builds with
plain g++ against the C-ABI, fails loudly without a GPU, and on a GPU leaves the same tracks and connections, bit
for bit, as the Python mirror (morph.PointTracker, stage_two_parameters, Parameters.add_point / move_point /
connect_point) over the same steps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from videomorphing_amd import capi, morph, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def track_points(tmp_path_factory, vmlib):
    exe = str(tmp_path_factory.mktemp("cppt") / "track_points")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "track_points.cpp"), "-o", exe,
                           "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    return exe


def _inputs(tmp_path, w, h, d):
    fr = [synth.make_video_pair(w, h, t, (0.5, 0.25), (1.5, -0.25)) for t in range(d)]
    v = [np.stack([np.repeat(np.clip(np.rint(f[k]), 0, 255).astype(np.uint8)[..., None], 3, -1) for f in fr]) for k in range(2)]
    np.stack([v[0], v[1]], 1).tofile(str(tmp_path / "fr.u8"))  # (d, 2, h, w, 3)
    # stage-1 connections (list, lx, ly, lz, rx, ry, rz): list 0 of three, list 1 of one
    cons = np.array([[0, 20, 30, 0, 24, 28, 1], [0, 40, 20, 3, 44, 22, 4], [0, 50, 40, 2, 48, 41, 2],
                     [1, 60, 25, 1, 62, 26, 3]], np.int32)
    cons.tofile(str(tmp_path / "cons.i32"))
    return v, cons


def test_track_facade_fails_loudly_without_gpu(track_points, vmlib, tmp_path):
    h = C.c_void_p()
    if vmlib.vm_ctx_create(0, C.byref(h)) == capi.VM_OK:
        vmlib.vm_ctx_destroy(h)
        pytest.skip("a HIP device is present")
    _inputs(tmp_path, 64, 48, 3)
    r = subprocess.run([track_points, "64", "48", "3", str(tmp_path / "fr.u8"), str(tmp_path / "cons.i32"), "4",
                        str(tmp_path / "o.i32")], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
    with pytest.raises(capi.VmError) as e:  # no context, so no tracker: the Python path fails the same way
        morph.Context(0)
    assert e.value.code == capi.VM_E_DEVICE


def _python_mirror(ctx, v, cons, w, h, d):
    tr = morph.PointTracker(ctx, v[0], v[1])
    Ps = morph.Parameters()
    for k, q in enumerate(cons.tolist()):
        Ps.lp.append([morph.Conp(q[1], q[2], q[3])])
        Ps.rp.append([morph.Conp(q[4], q[5], q[6])])
        while len(Ps.cnt) <= q[0]:
            Ps.cnt.append([])
        Ps.cnt[q[0]].append(morph.Connect((k, 0), (k, 0)))
    P = morph.stage_two_parameters(Ps, tr)
    a = P.add_point(0, w // 3, h // 2, d - 1, tr)
    b = P.add_point(1, w // 2, h // 2, d // 2, tr)
    P.move_point(0, a, 0, w // 2, h // 3, tr)
    P.connect_point(a, b)
    out = [len(P.lp), len(P.rp), len(P.cnt)]
    for side in (P.lp, P.rp):
        for track in side:
            for c in track:
                out += list(c.p) + [int(np.float32(c.weight).view(np.int32))]
    for row in P.cnt:
        out.append(len(row))
        for c in row:
            out += [c.li[0], c.li[1], c.ri[0], c.ri[1]]
    return np.array(out, np.int32)


@pytest.mark.gpu
def test_track_facade_matches_python_mirror(track_points, gpu_ctx, tmp_path):
    w, h, d = 96, 64, 5
    v, cons = _inputs(tmp_path, w, h, d)
    out = tmp_path / "o.i32"
    r = subprocess.run([track_points, str(w), str(h), str(d), str(tmp_path / "fr.u8"), str(tmp_path / "cons.i32"),
                        str(len(cons)), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(str(out), np.int32)
    want = _python_mirror(gpu_ctx, v, cons, w, h, d)
    assert got[:3].tolist() == [3, 3, 3]  # two converted lists plus one added track per side, plus their new connection list
    assert np.array_equal(got, want)
