"""The residency of the kernels of videomorphing_amd/csrc/vm_multiband.hip as the compiler reports it, kept as a promise
(DESIGN 3.19): every instantiation is there, none has scratch or AGPRs, each window kernel's LDS is exactly the windows it
stages, and its registers allow the waves per SIMD that its own LDS and the CU's wave slots allow -- the rule of
tests/test_vshutter_resources.py.  The unit is cross-compiled with the build's own flags (no GPU) and the compiler's
resource remarks are read; nothing is run."""
import re

import pytest

from kernel_resources import unit_usage

LDS_PER_CU = 160 * 1024         # bytes
WAVE_SLOTS = 32                 # per CU, four SIMDs
REGISTER_FILE, GRANULE = 512, 8     # VGPRs + AGPRs per lane and SIMD; the allocation granule
CHAIN_WINDOW = (32 + 2 * 10 + 1) * (16 + 2 * 10 + 1) * 8    # vm_chain.h: WW x WH cells of float2
TW, TH = 32, 8                  # vm_multiband.hip: a workgroup's tile
REDUCE_WINDOW = (2 * TW + 3) * (2 * TH + 3) * 4
COARSE_WINDOW = (TW // 2 + 2) * (TH // 2 + 2) * 4


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel: {"VGPRs": n, "ScratchSize [bytes/lane]": n, ...}} of every kernel of the unit"""
    return unit_usage("vm_multiband.hip", tmp_path_factory.mktemp("mbres"))


def _family(usage, name):
    return [k for k in usage if re.search(r"\d+%s(E|I)" % name, k)]


def _ints(k):
    """the template arguments of a mangled kernel name: L b <0|1> E -> bool, L i <n> E -> int (n1: -1)"""
    return [(t == "b" and v == "1") if t == "b" else -int(v[1:]) if v[0] == "n" else int(v) for t, v in re.findall(r"L([bi])(n?\d+)E", k)]


def test_every_instantiation_is_there_and_none_spills(usage):
    plain, win = _family(usage, "k_mb_warp"), _family(usage, "k_mb_warp_win")
    collapse, reduce_, base = _family(usage, "k_mb_collapse"), _family(usage, "k_mb_reduce"), _family(usage, "k_mb_base")
    channels = (1, 2, 3, 4, -1)                     # layers of 1..4 channels, the canvases
    assert sorted(map(_ints, plain)) == sorted([c, r] for c in channels for r in (False, True))
    assert sorted(map(_ints, win)) == sorted([u, c, r] for u in (False, True) for c in channels for r in (False, True))
    # planes above level 0 and texels at level 0 for 1..4 channels; bytes for the canvases' three
    assert sorted(map(_ints, collapse)) == sorted([[c, o] for c in (1, 2, 3, 4) for o in (0, 1)] + [[3, 2]])
    assert len(reduce_) == 1 and len(base) == 1 and len(usage) == 10 + 20 + 9 + 2, sorted(usage)
    for k, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["AGPRs"] == 0, (k, u)


def test_lds_is_the_staged_windows(usage):
    for k in _family(usage, "k_mb_warp_win"):
        has_u, _, rates = _ints(k)
        n = 1 + has_u + rates           # v, the path, the rates; a window is 8 bytes short of a multiple of 16 and the next one is aligned
        assert usage[k]["LDS Size [bytes/block]"] == CHAIN_WINDOW * n + 8 * (n - 1), (k, usage[k])
    for k in _family(usage, "k_mb_collapse"):
        assert usage[k]["LDS Size [bytes/block]"] == 3 * _ints(k)[0] * COARSE_WINDOW, (k, usage[k])
    assert usage[_family(usage, "k_mb_reduce")[0]]["LDS Size [bytes/block]"] == REDUCE_WINDOW
    for k in _family(usage, "k_mb_warp") + _family(usage, "k_mb_base"):
        assert usage[k]["LDS Size [bytes/block]"] == 0, (k, usage[k])


def test_window_kernels_registers_allow_what_their_lds_allows(usage):
    """workgroups per CU = min(LDS per CU / LDS per workgroup, wave slots / waves per workgroup); the registers of a wave are
    allocated in granules of 8 out of 512 per lane and SIMD, at most eight waves"""
    for k in _family(usage, "k_mb_warp_win") + _family(usage, "k_mb_collapse") + _family(usage, "k_mb_reduce"):
        u = usage[k]
        waves = (512 if "warp_win" in k else TW * TH) // 64
        workgroups = min(LDS_PER_CU // u["LDS Size [bytes/block]"], WAVE_SLOTS // waves)
        by_lds = workgroups * waves // 4
        alloc = -(-(u["VGPRs"] + u["AGPRs"]) // GRANULE) * GRANULE
        by_registers = min(8, REGISTER_FILE // alloc)
        assert by_registers >= by_lds, (k, u, by_registers, by_lds)
