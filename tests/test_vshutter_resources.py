"""The residency of the kernels of videomorphing_amd/csrc/vm_vshutter.hip as the compiler reports it, kept as a promise
(DESIGN 3.14): every instantiation is there, none has scratch or AGPRs, the window kernels' LDS is the windows they
stage -- one without a path and without rates, two with either, three with both -- and a window kernel's registers
allow at least the waves per SIMD that its own LDS and the CU's wave slots allow.  What the two loops hold in registers
is the compiler's decision (per_sample() in vm_shutter_tail.h is there for that), so a compiler that decides otherwise
shows here and not in a timing.  The unit is cross-compiled with the build's own flags (no GPU) and the compiler's
resource remarks are read; nothing is run."""
import re

import pytest

from kernel_resources import unit_usage

LDS_PER_CU = 160 * 1024         # bytes
WAVE_SLOTS = 32                 # per CU, four SIMDs
WAVES_PER_WORKGROUP = 512 // 64
REGISTER_FILE, GRANULE = 512, 8     # VGPRs + AGPRs per lane and SIMD; the allocation granule
WINDOW = 8 * 53 * 37            # bytes of one staged window of float2 cells (vm_chain.h: WW x WH)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel: {"VGPRs": n, "ScratchSize [bytes/lane]": n, ...}} of every kernel of the unit"""
    return unit_usage("vm_vshutter.hip", tmp_path_factory.mktemp("vshres"))


def _split(usage):
    win = [k for k in usage if "k_vblur_win" in k]
    return win, [k for k in usage if "k_vblur" in k and k not in win]


def _flags(k):
    """(HAS_U, RATES) of a window kernel's mangled name: k_vblur_winILb<HAS_U>ELi<C>ELb<RATES>EE"""
    m = re.search(r"k_vblur_winILb([01])ELi(?:n?\d+)ELb([01])EE", k)
    assert m, k
    return m.group(1) == "1", m.group(2) == "1"


def test_every_instantiation_is_there_and_none_spills(usage):
    win, plain = _split(usage)
    # HAS_U x (1..4, CANVAS) x RATES; (1..4, CANVAS) x RATES
    assert len(win) == 20 and len(plain) == 10, sorted(usage)
    assert len(usage) == 30, sorted(usage)
    assert sorted(_flags(k) for k in win) == sorted([(u, r) for u in (False, True) for r in (False, True)] * 5)
    assert sum("ELb1EE" in k for k in plain) == 5 and sum("ELb0EE" in k for k in plain) == 5, plain
    for k in win + plain:
        assert usage[k]["ScratchSize [bytes/lane]"] == 0 and usage[k]["AGPRs"] == 0, (k, usage[k])


def test_window_kernels_registers_allow_what_their_lds_allows(usage):
    """workgroups per CU = min(LDS per CU / LDS per workgroup, wave slots / waves per workgroup); the registers of a
    wave are allocated in granules of 8 out of 512 per lane and SIMD, at most eight waves"""
    win, _ = _split(usage)
    for k in win:
        u = usage[k]
        lds = u["LDS Size [bytes/block]"]
        workgroups = min(LDS_PER_CU // lds, WAVE_SLOTS // WAVES_PER_WORKGROUP)
        by_lds = workgroups * WAVES_PER_WORKGROUP // 4
        alloc = -(-(u["VGPRs"] + u["AGPRs"]) // GRANULE) * GRANULE
        by_registers = min(8, REGISTER_FILE // alloc)
        assert by_registers >= by_lds, (k, u, by_registers, by_lds)


def test_lds_sizes_are_the_design_tables(usage):
    """windows of 53 x 37 cells: v, u with a path, (G, K) under a schedule; a window that is not staged is one cell.
    15688 / 31384 bytes without rates, 31384 / 47080 with"""
    assert WINDOW == 15688
    win, plain = _split(usage)
    for k in win:
        has_u, rates = _flags(k)
        windows = 1 + has_u + rates
        want = {1: 15688, 2: 31384, 3: 47080}[windows]
        assert want == windows * WINDOW + (windows - 1) * 8       # (each further window begins on 16 bytes)
        assert usage[k]["LDS Size [bytes/block]"] == want, (k, usage[k])
    for k in plain:
        assert usage[k]["LDS Size [bytes/block]"] == 0, (k, usage[k])
