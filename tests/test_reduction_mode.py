"""vm_set_reduction (VM_REDUCE_ATOMIC / VM_REDUCE_ORDERED) without a GPU: the entry point through every layer -- header,
library, ctypes binding, Python wrapper, C++ facade -- its refusals, the VM_REDUCTION switch, and the ordered fold's
arrival counting and fold order restated on the host.  What the mode DOES is in tests/test_gpu_reduction_mode.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

import reduction_cases as RC
from videomorphing_amd import capi, morph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_reduction_is_declared_exported_and_bound(vmlib):
    src = open(os.path.join(ROOT, "include", "vmorph.h")).read()
    assert re.search(r"\bint\s+vm_set_reduction\(vm_ctx \*ctx, int mode\);", src)
    assert re.search(r"#define VM_REDUCE_ATOMIC 0\b", src) and re.search(r"#define VM_REDUCE_ORDERED 1\b", src)
    assert "PoissonExt.cpp:321-329" in src[src.index("vm_set_commit_order(vm_ctx"):src.index("vm_set_reduction(vm_ctx")]
    assert "vm_set_reduction" in capi.SYMBOLS and hasattr(vmlib, "vm_set_reduction")
    assert vmlib.vm_set_reduction.argtypes == [C.c_void_p, C.c_int]
    assert (capi.REDUCE_ATOMIC, capi.REDUCE_ORDERED) == (0, 1)


def test_set_reduction_refuses_null_and_unknown_modes_before_touching_anything(vmlib):
    assert vmlib.vm_host_unregister(None) == capi.VM_E_INVALID          # a message that is not this call's
    stale = vmlib.vm_last_error()
    for mode in (0, 1):
        assert vmlib.vm_set_reduction(None, mode) == capi.VM_E_INVALID
        assert b"vm_set_reduction" in vmlib.vm_last_error() and b"NULL" in vmlib.vm_last_error() != stale
    # a mode outside 0..1 is refused before the handle is looked at: 4 KB of zeros stand in for a context
    fake = C.create_string_buffer(4096)
    for mode in (2, -1, 7):
        assert vmlib.vm_set_reduction(C.cast(fake, C.c_void_p), mode) == capi.VM_E_INVALID
        assert ("mode %d" % mode).encode() in vmlib.vm_last_error()
    assert fake.raw == bytes(4096)


def test_python_wrapper_and_inheritance_exist():
    assert callable(morph.Context.set_reduction)
    assert (morph.REDUCE_ATOMIC, morph.REDUCE_ORDERED) == (0, 1)
    import inspect
    assert "others[0].reduction" in inspect.getsource(morph.context_beside)


def test_unknown_vm_reduction_value_fails_ctx_create(vmlib):
    """VM_REDUCTION=ordered|atomic sets a context's initial mode; anything else fails vm_ctx_create with VM_E_INVALID and
    names the value (checked before a device is looked for: in a child process, the variable is read per call)"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from videomorphing_amd import capi; L = capi.load(); h = C.c_void_p(); "
            "rc = L.vm_ctx_create(0, C.byref(h)); print(rc, bool(h.value), L.vm_last_error().decode())" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VM_REDUCTION="sorted"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[:2] == [str(capi.VM_E_INVALID), "False"] and "VM_REDUCTION=sorted" in r.stdout


def test_cpp_setter_compiles_with_gxx(tmp_path, vmlib):
    libdir = os.path.dirname(capi.LIB_PATH)
    src = tmp_path / "red.cpp"
    src.write_text('#include <cstdio>\n#include "vmorph/pyramid.hpp"\n'
                   'int main() { try { vmorph::Context c(0); c.set_reduction(VM_REDUCE_ORDERED); c.set_reduction(VM_REDUCE_ATOMIC); }\n'
                   'catch (const std::exception &e) { fprintf(stderr, "%s\\n", e.what()); return 1; } return 0; }\n')
    for source, exe in ((str(src), "red"), (os.path.join(ROOT, "examples", "pipeline_shard.cpp"), "pipeline_shard")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), source, "-o", str(tmp_path / exe),
                               "-L", libdir, "-lvmorph_hip", "-Wl,-rpath," + libdir, "-lpthread"])
    ex = open(os.path.join(ROOT, "examples", "pipeline_shard.cpp")).read()
    assert "--ordered" in ex and "set_reduction(VM_REDUCE_ORDERED)" in ex
    r = subprocess.run([str(tmp_path / "pipeline_shard")], capture_output=True, text=True)
    assert r.returncode == 2 and "--ordered" in r.stderr


def test_ordered_fold_restated_on_the_host():
    """the arrival counting and the fold order of vm_mgb.hip's ordered mode: whatever the arrival order, and however many
    workgroups the launch holds beyond the system's own n (the batch's maximum), exactly one workgroup folds each group,
    after every partial of the group is published; the tickets stand at zero again; and the totals -- the device's and
    the host's -- have the same bits.  With sums that are NOT associative in double, so an order-dependent fold shows."""
    rng = np.random.default_rng(7)
    for n in (1, 31, 32, 33, 64, 1000, 3294, 3312):
        parts = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).astype(np.float64)
        seen_dev, seen_host = set(), set()
        tickets = None
        for trial in range(6):
            grid = n + (0, 1, 57, 500, 0, 3)[trial]
            arrival = list(range(grid))
            if trial == 4:
                arrival.reverse()
            elif trial:
                rng.shuffle(arrival)
            gsum, ng, folders, tickets = RC.produce(parts, n, grid, arrival, tickets)        # the tickets of the launch before
            assert ng == (n + 31) // 32 and all(t == 0 for t in tickets)
            assert all(f is not None and f < n and f // RC.GROUP == g for g, f in enumerate(folders))
            for g in range(ng):                  # a group's sum: its partials in ascending order from zero
                s = np.float64(0)
                for j in range(g * 32, min(n, g * 32 + 32)):
                    s = s + parts[j]
                assert s.tobytes() == gsum[g].tobytes()
            seen_dev.add(RC.consume_device(gsum, ng).tobytes())
            seen_host.add(RC.consume_host(gsum, ng).tobytes())
        assert len(seen_dev) == 1 and len(seen_host) == 1, n
    # ... while the default's arrival-order sum does depend on the order (what the mode removes)
    parts = (rng.standard_normal(3294) * 10.0 ** rng.integers(-8, 9, 3294)).astype(np.float64)
    sums = set()
    for _ in range(8):
        s = np.float64(0)
        for i in rng.permutation(3294):
            s = s + parts[i]
        sums.add(s.tobytes())
    assert len(sums) > 1


def test_ordered_storage_fits_every_producer(tmp_path):
    """the room the solver gives a system (vm_mgb_plan.h: MgbOrdLayout, asked of the header itself) -- cap producing
    workgroups in gcap groups -- covers the streaming kernels' groups of four blocks and the tile kernels' tiles, whatever
    the type map (from the grid alone, as the host states it)"""
    src = tmp_path / "ord.cpp"
    src.write_text('#include "vm_mgb_plan.h"\n#include <cstdio>\n'
                   'int main() { for (int gx, gy; scanf("%d %d", &gx, &gy) == 2;) { const MgbOrdLayout Y(gx, gy); printf("%d %d\\n", Y.cap, Y.gcap); } }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "videomorphing_amd", "csrc"), str(src), "-o", str(tmp_path / "ord")])
    grids = [((w + 63) // 64, (h + 3) // 4) for w, h in ((2304, 1464), (1920, 1080), (64, 4), (65, 5), (2, 2), (510, 300), (4096, 2200))]
    out = subprocess.run([str(tmp_path / "ord")], input="".join("%d %d\n" % g for g in grids), capture_output=True, text=True, check=True).stdout
    caps = [tuple(int(x) for x in l.split()) for l in out.splitlines()]
    assert len(caps) == len(grids)
    for (gx, gy), (cap, gcap) in zip(grids, caps):
        for nblocks in (0, 1, gx * gy // 2, gx * gy):
            assert (nblocks + 3) // 4 <= cap
        assert gx * ((gy + 3) // 4) <= cap          # every tile of the grid
        assert gcap * RC.GROUP >= cap > (gcap - 1) * RC.GROUP
    assert grids[0] == (36, 366) and caps[0][0] == 3312
    assert max((36 * 366 + 3) // 4, 36 * 92) == 3312
