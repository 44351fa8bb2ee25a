"""The residency of the kernels of videomorphing_amd/csrc/vm_tshutter.hip as the compiler reports it, kept as a promise
(DESIGN 3.12): every instantiation is there, none has scratch or AGPRs, and a window kernel's registers allow at least
the waves per SIMD that its own LDS windows and the CU's wave slots allow -- three windows with a path (two workgroups
less per CU than the uniform shutter), two without.  What the sample loop holds in registers is the compiler's decision
(per_sample() in vm_shutter_tail.h is there for that), so a compiler that decides otherwise shows here and not in a
timing.  The unit is cross-compiled with the build's own flags (no GPU) and the compiler's resource remarks are read;
nothing is run."""
import pytest

from kernel_resources import unit_usage

LDS_PER_CU = 160 * 1024         # bytes
WAVE_SLOTS = 32                 # per CU, four SIMDs
WAVES_PER_WORKGROUP = 512 // 64
REGISTER_FILE, GRANULE = 512, 8     # VGPRs + AGPRs per lane and SIMD; the allocation granule


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel: {"VGPRs": n, "ScratchSize [bytes/lane]": n, ...}} of every kernel of the unit"""
    return unit_usage("vm_tshutter.hip", tmp_path_factory.mktemp("tshres"))


def _split(usage):
    win = [k for k in usage if "k_tblur_win" in k]
    return win, [k for k in usage if "k_tblur" in k and k not in win]


def test_every_instantiation_is_there_and_none_spills(usage):
    win, plain = _split(usage)
    assert len(win) == 10 and len(plain) == 5, sorted(usage)      # HAS_U x (1..4, CANVAS); (1..4, CANVAS)
    assert len(usage) == 15 and not [k for k in usage if "k_shutter" in k], sorted(usage)
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
    """three windows of 53 x 37 cells with a path, two without (win_u is then one cell): 47080 and 31384 bytes, six and
    eight waves per SIMD"""
    win, plain = _split(usage)
    for k in win:
        has_u = "ILb1E" in k
        assert "ILb1E" in k or "ILb0E" in k, k
        assert usage[k]["LDS Size [bytes/block]"] == (47080 if has_u else 31384), (k, usage[k])
    for k in plain:
        assert usage[k]["LDS Size [bytes/block]"] == 0, (k, usage[k])
