"""What the layers' extension costs in registers, as the compiler reports it: the kernels of
videomorphing_amd/csrc/vm_layer_ext.hip use no scratch and no LDS, and the layer instantiations of the render kernels --
k_warp / k_warp_win and the kernels that include vm_shutter_tail.h, whose taps now take the layers' own grid (lw, lh) and
offset (lexf) -- keep their LDS size, keep zero scratch and stay below 64 VGPRs wherever they were below 64 before the
extension existed.  The units are cross-compiled with the build's own flags (no GPU) and the compiler's resource remarks
are read; nothing is run.

The plain viewport kernels take their sample counts anew per sample for that (vm_viewport.hip): held across the chain
as floats beside the layers' grid, they put k_viewport<2> at 64."""
import re

import pytest

from kernel_resources import unit_usage

WINDOW = 8 * 53 * 37            # bytes of one staged window of float2 cells (vm_chain.h: WW x WH)
UNITS = ["vm_warp.hip", "vm_shutter.hip", "vm_tshutter.hip", "vm_viewport.hip", "vm_vshutter.hip"]
# the layer instantiations that stood at 64 VGPRs or above before the extension (all others were below): the plain forms
# of the shutters, the 3- and 4-channel plain viewport, and the window forms that stage three windows
AT_OR_ABOVE_64_BEFORE = [r"\dk_shutterILi", r"\dk_tblurILi", r"k_tblur_winILb1", r"k_viewportILi[34]E", r"\dk_vblurILi",
                         r"k_vblur_winILb1ELi\dELb1"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lextres")
    return {u: unit_usage(u, tmp) for u in UNITS + ["vm_layer_ext.hip"]}


def _layer_kernels(usage):
    """[(unit, mangled name)] of the instantiations with C in 1..4"""
    return [(u, k) for u in UNITS for k in sorted(usage[u]) if re.search(r"(?:k_warp|k_shutter|k_tblur|k_viewport|k_vblur)(?:_win)?I(?:Lb[01]E)?Li[1-4]E", k)]


def _windows(k):
    """how many windows a kernel stages: v, u with a path, (G, K) under a schedule; none in the plain forms"""
    m = re.search(r"_winILb([01])ELi\d(?:ELb([01]))?E", k)
    if not m:
        return 0
    rates = "k_tblur_win" in k or m.group(2) == "1"
    return 1 + (m.group(1) == "1") + rates


def test_the_new_kernels_use_no_scratch(usage):
    mine = usage["vm_layer_ext.hip"]
    # canvas and fill for 1..4 channels, the type map, set-up and paste
    assert len(mine) == 11 and sum("k_lx_fill" in k for k in mine) == 4 and sum("k_lx_canvas" in k for k in mine) == 4, sorted(mine)
    for k, u in mine.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0 and u["AGPRs"] == 0, (k, u)
        assert u["VGPRs"] <= 64, (k, u)


def test_layer_instantiations_keep_their_lds_and_have_no_scratch(usage):
    kernels = _layer_kernels(usage)
    # warp: (2 window forms + plain) x 4 x RATES; shutter, tshutter, viewport: (2 + 1) x 4; vshutter: (2 + 1) x 4 x RATES
    assert len(kernels) == 24 + 12 + 12 + 12 + 24, len(kernels)
    for u, k in kernels:
        n = _windows(k)
        want = n * WINDOW + max(n - 1, 0) * 8       # (each further window begins on 16 bytes)
        assert usage[u][k]["LDS Size [bytes/block]"] == want, (k, usage[u][k])
        assert usage[u][k]["ScratchSize [bytes/lane]"] == 0 and usage[u][k]["AGPRs"] == 0, (k, usage[u][k])


def test_layer_instantiations_stay_below_64_registers_where_they_were(usage):
    over = []
    for u, k in _layer_kernels(usage):
        if any(re.search(p, k) for p in AT_OR_ABOVE_64_BEFORE):
            continue
        if usage[u][k]["VGPRs"] >= 64:
            over.append((k, usage[u][k]["VGPRs"]))
    assert not over, over
