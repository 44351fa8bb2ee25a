"""The residency of the viewport kernels (videomorphing_amd/csrc/vm_viewport.hip) as the compiler reports it, kept as a
promise: DESIGN 3.13 holds the window kernels below the 64 VGPRs at which a workgroup of 512 threads loses residency, and
every kernel of the unit free of scratch.  How many registers the sample loop takes depends on what the compiler hoists
out of it (per_sample() in the unit is there for that), so a compiler that decides otherwise shows here and not in a
timing.  The unit is cross-compiled with the build's own flags (no GPU) and the compiler's resource remarks are read;
nothing is run."""
import pytest

from kernel_resources import unit_usage


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel: {"VGPRs": n, "ScratchSize [bytes/lane]": n, ...}} of every kernel of the unit"""
    return unit_usage("vm_viewport.hip", tmp_path_factory.mktemp("vpres"))


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
