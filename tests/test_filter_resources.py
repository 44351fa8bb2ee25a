"""The residency of the kernels of videomorphing_amd/csrc/vm_filter.hip as the compiler reports it, kept as a promise
(DESIGN 3.18): every instantiation is there, none has scratch or AGPRs, the window kernels' LDS is the windows they stage,
and for the canvases and for 1 and 2 channels a window kernel's registers allow the waves per SIMD that its own LDS and
the CU's wave slots allow -- the rule of tests/test_vshutter_resources.py, which here means at most 64 VGPRs.  For 3 and 4
channels the row-by-row tail of vm_filter_tap.h reaches 72 VGPRs (seven waves); fetching a row in two halves reaches 59 / 62
and was measured slower (profiles/filtered.md), so those kernels are held to 128.  The unit is cross-compiled
with the build's own flags (no GPU) and the compiler's resource remarks are read; nothing is run."""
import re

import pytest

from kernel_resources import unit_usage

LDS_PER_CU = 160 * 1024         # bytes
WAVE_SLOTS = 32                 # per CU, four SIMDs
WAVES_PER_WORKGROUP = 512 // 64
REGISTER_FILE, GRANULE = 512, 8     # VGPRs + AGPRs per lane and SIMD; the allocation granule


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel: {"VGPRs": n, "ScratchSize [bytes/lane]": n, ...}} of every kernel of the unit"""
    return unit_usage("vm_filter.hip", tmp_path_factory.mktemp("fltres"))


def _split(usage):
    win = [k for k in usage if "k_fview_win" in k]
    return win, [k for k in usage if "k_fview" in k and k not in win]


def _args(k):
    """(HAS_U, C) of a window kernel's mangled name: k_fview_winILb<HAS_U>ELi<C>EE (C = n1: the canvases)"""
    m = re.search(r"k_fview_winILb([01])ELi(n?\d+)EE", k)
    assert m, k
    return m.group(1) == "1", m.group(2)


def test_every_instantiation_is_there_and_none_spills(usage):
    win, plain = _split(usage)
    assert len(win) == 10 and len(plain) == 5 and len(usage) == 15, sorted(usage)      # HAS_U x (1..4, CANVAS); (1..4, CANVAS)
    assert sorted(_args(k) for k in win) == sorted((u, c) for u in (False, True) for c in ("1", "2", "3", "4", "n1"))
    for k in win + plain:
        assert usage[k]["ScratchSize [bytes/lane]"] == 0 and usage[k]["AGPRs"] == 0, (k, usage[k])


def test_lds_is_the_staged_windows(usage):
    win, plain = _split(usage)
    for k in win:
        assert usage[k]["LDS Size [bytes/block]"] == (31384 if _args(k)[0] else 15688), (k, usage[k])
    for k in plain:
        assert usage[k]["LDS Size [bytes/block]"] == 0, (k, usage[k])


def test_window_kernels_registers_allow_what_their_lds_allows(usage):
    """workgroups per CU = min(LDS per CU / LDS per workgroup, wave slots / waves per workgroup); the registers of a
    wave are allocated in granules of 8 out of 512 per lane and SIMD, at most eight waves.  The canvases, 1 and 2 channels:
    what the LDS allows, eight waves; 3 and 4 channels: at most 128 VGPRs, the four waves of one resident workgroup"""
    win, _ = _split(usage)
    for k in win:
        u = usage[k]
        workgroups = min(LDS_PER_CU // u["LDS Size [bytes/block]"], WAVE_SLOTS // WAVES_PER_WORKGROUP)
        by_lds = workgroups * WAVES_PER_WORKGROUP // 4
        alloc = -(-(u["VGPRs"] + u["AGPRs"]) // GRANULE) * GRANULE
        by_registers = min(8, REGISTER_FILE // alloc)
        assert by_lds == 8, (k, u)
        if _args(k)[1] in ("3", "4"):
            assert u["VGPRs"] <= 128, (k, u)
        else:
            assert u["VGPRs"] <= 64 and by_registers >= by_lds, (k, u, by_registers, by_lds)
