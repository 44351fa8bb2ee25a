"""The residency of the carry kernels (videomorphing_amd/csrc/vm_carry.hip) as the compiler reports it, kept as a promise
(DESIGN 3.17): every instantiation is there and free of scratch, and the loop over the to-times costs the window form no
residency -- no k_motion_win sits in a lower wave-residency class than the maps kernel of vm_warp.hip that walks the same
chain, k_warp_win<HAS_U, 0, RATES> with the same two flags, read from that unit in the same test.  Both units are
cross-compiled with the build's own flags (no GPU) and the compiler's resource remarks are read; nothing is run."""
import pytest

from kernel_resources import unit_usage


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("carryres")
    return unit_usage("vm_carry.hip", tmp), unit_usage("vm_warp.hip", tmp)


def _flags(b):
    return "Lb1E" if b else "Lb0E"


def _waves_by_registers(u):
    """the waves per SIMD the allocated VGPRs + AGPRs of a kernel admit on gfx950: 512 per lane and SIMD, granules of 8"""
    regs = (u["VGPRs"] + u["AGPRs"] + 7) // 8 * 8
    return min(8, 512 // max(regs, 8))


def test_every_instantiation_is_there_and_none_spills(usage):
    carry, _ = usage
    points = [k for k in carry if "k_carry_points" in k]
    win = [k for k in carry if "k_motion_win" in k]
    plain = [k for k in carry if "k_motion" in k and k not in win]
    assert len(points) == 4 and len(win) == 4 and len(plain) == 2, sorted(carry)      # HAS_U x RATES; HAS_U x RATES; RATES
    for k in points + win + plain:
        assert carry[k]["ScratchSize [bytes/lane]"] == 0, (k, carry[k])
    for k in points + plain:
        assert carry[k]["LDS Size [bytes/block]"] == 0, (k, carry[k])


def test_window_kernels_keep_the_maps_kernels_residency(usage):
    carry, warp = usage
    for has_u in (False, True):
        for rates in (False, True):
            mine = [k for k in carry if "k_motion_winI%s%sE" % (_flags(has_u), _flags(rates)) in k]
            maps = [k for k in warp if "k_warp_winI%sLi0E%sE" % (_flags(has_u), _flags(rates)) in k]
            assert len(mine) == 1 and len(maps) == 1, (has_u, rates, sorted(carry), sorted(warp))
            a, b = carry[mine[0]], warp[maps[0]]
            assert a["Occupancy [waves/SIMD]"] >= b["Occupancy [waves/SIMD]"], (a, b)
            assert _waves_by_registers(a) >= _waves_by_registers(b), (a, b)
            assert a["LDS Size [bytes/block]"] == b["LDS Size [bytes/block]"], (a, b)
