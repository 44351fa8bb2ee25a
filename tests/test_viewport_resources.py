"""The residency of the viewport kernels (videomorphing_amd/csrc/vm_viewport.hip) as the compiler reports it, kept as a
promise: DESIGN 3.13 holds the window kernels below the 64 VGPRs at which a workgroup of 512 threads loses residency, and
every kernel of the unit free of scratch.  How many registers the sample loop takes depends on what the compiler hoists
out of it (per_sample() in the unit is there for that), so a compiler that decides otherwise shows here and not in a
timing.  The unit is cross-compiled with the build's own flags (no GPU) and the compiler's resource remarks are read;
nothing is run."""
import os
import re
import subprocess

import pytest

from videomorphing_amd import build

SRC = os.path.join(build.CSRC, "vm_viewport.hip")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel: {"VGPRs": n, "ScratchSize [bytes/lane]": n, ...}} of every kernel of the unit"""
    obj = str(tmp_path_factory.mktemp("vpres") / "vm_viewport.o")
    extra = [e for s, _, e in build.UNITS if s == "vm_viewport.hip"][0]
    assert "-ffp-contract=off" in extra
    r = subprocess.run([build._hipcc()] + build.COMMON + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", obj],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z][^:]*): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            out[name] = {}
        elif name:
            out[name][m.group(2).strip()] = int(m.group(3))
    return out


def test_every_instantiation_is_there_and_none_spills(usage):
    win = [k for k in usage if "k_viewport_win" in k]
    plain = [k for k in usage if "k_viewport" in k and k not in win]
    assert len(win) == 10 and len(plain) == 5, sorted(usage)      # HAS_U x (1..4, CANVAS); (1..4, CANVAS)
    for k in win + plain:
        assert usage[k]["ScratchSize [bytes/lane]"] == 0, (k, usage[k])


def test_window_kernels_stay_below_64_vgprs(usage):
    for k, u in usage.items():
        if "k_viewport_win" in k:
            assert u["VGPRs"] < 64 and u["AGPRs"] == 0, (k, u)
            assert u["LDS Size [bytes/block]"] in (15688, 31384), (k, u)
