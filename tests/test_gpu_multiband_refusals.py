"""The multiband calls in the render calls' one order of refusals (include/vmorph.h), as
tests/test_gpu_render_refusals.py holds it for the vm_render_* ones: after the handle a NULL output (a call that downloads),
the arguments -- bands NULL, its level count, the coarsest level, a sharp entry, the ease --, the frame's state (no schedule,
then no layers), the pitch.  One fault answers with its code and its message under the call's own name; of two faults at once
the earlier one answers; the _dev twin cannot carry a NULL output or a pitch and answers for what is left.  Every call here
is refused by a check on the host, or is a good call, and the frames render afterwards what they rendered before.

The frames are 33 x 7 with ex = 3, as in the refusal tests of the families: two levels leave 9 x 2, three would leave 5 x 1."""
import ctypes as C
import itertools

import numpy as np
import pytest

from render_cases import field as _field, frame as _frame, layers as _layers, same_bits as _same
from videomorphing_amd import capi, transition
from videomorphing_amd.multiband import Bands

pytestmark = pytest.mark.gpu

W, H, EX, CH = 33, 7, 3, 2
OK, ST, INV = capi.VM_OK, capi.VM_E_STATE, capi.VM_E_INVALID
CALLS = ["vm_frame_render_multiband", "vm_frame_render_multiband_layers", "vm_frame_render_multiband_transition",
         "vm_frame_render_multiband_transition_layers"]
# fault -> (its place in the order, the code, what the message says)
FAULTS = {
    "null_output": (0, INV, "output is NULL"),
    "null_bands": (1, INV, "bands is NULL"),
    "levels": (2, INV, "9 levels"),
    "coarsest": (3, INV, "coarsest level of 5 x 1"),
    "sharp": (4, INV, "sharp[1]"),
    "ease": (5, INV, "ease 2"),
    "no_schedule": (6, ST, "holds no schedule"),
    "no_layers": (7, ST, "holds no layers"),
    "pitch": (8, INV, "below the row"),
}
BANDS_FAULTS = ("null_bands", "levels", "coarsest")      # one vm_bands carries one of these (and a sharp entry beside it)


def _expressible(name):
    out = ["null_output", "null_bands", "levels", "coarsest", "sharp", "pitch"]
    out += ["ease", "no_schedule"] if "transition" in name else []
    return out + (["no_layers"] if name.endswith("_layers") else [])


def _bands(faults):
    b = Bands.sharpen(2, 4).struct()
    if "levels" in faults:
        b.levels = 9
    if "coarsest" in faults:
        b.levels = 3
        b.sharp[3] = 1.0
    if "sharp" in faults:
        b.sharp[1] = 0.5
    return b


@pytest.fixture(scope="module")
def frames(gpu_ctx):
    v, u = _field(W, H, "smooth", True)
    out = {}
    for sched, lay in itertools.product((False, True), repeat=2):
        fr = _frame(gpu_ctx, W, H, EX, v, u, (transition.wipe(W, H), transition.radial(W, H)) if sched else None)
        if lay:
            fr.upload_layers(_layers(W, H, CH, 1), _layers(W, H, CH, 2))
        out[sched, lay] = fr
    yield out
    for fr in out.values():
        fr.close()


def _state(fr, sched, lay):
    out = [fr.download_v(), fr.download_qpath(), fr.download_ext(1), fr.download_ext(2), fr.render_halfway(0.3, 0.35, 1)]
    if sched:
        out += list(fr.transition_maps(0.4, capi.EASE_SMOOTH))
    if lay:
        out.append(fr.render_layers(0.3, 0.35, 1))
    return out


def _call(frames, name, faults, dev):
    """(code, message) of `name` (dev: of its twin) with good arguments and the given faults"""
    fr = frames["no_schedule" not in faults, "no_layers" not in faults]
    L = fr._L
    b = _bands(faults)
    head = (None if "null_bands" in faults else C.byref(b),)
    args = (0.4, 2 if "ease" in faults else capi.EASE_SMOOTH) if "transition" in name else (0.3, 0.35)
    host = np.zeros(64 * 64 * 4, np.float32)
    ms = C.c_float(0)
    if dev:
        rc = getattr(L, name + "_dev")(fr._h, *head, *args, C.byref(ms))
    else:
        row = W * (CH if name.endswith("_layers") else 3)
        rc = getattr(L, name)(fr._h, *head, *args, None if "null_output" in faults else host.ctypes.data, row - 1 if "pitch" in faults else 0)
    return rc, L.vm_last_error().decode()


def test_one_fault_at_a_time(frames):
    before = {k: _state(fr, *k) for k, fr in frames.items()}
    for name in CALLS:
        assert _call(frames, name, (), False)[0] == OK and _call(frames, name, (), True)[0] == OK, name
        for fault in _expressible(name):
            for dev in (False, True):
                if dev and fault in ("null_output", "pitch"):
                    continue
                rc, msg = _call(frames, name, (fault,), dev)
                assert rc == FAULTS[fault][1], (name, fault, dev, msg)
                assert msg.startswith(name + ("_dev: " if dev else ": ")) and FAULTS[fault][2] in msg, (name, fault, dev, msg)
    # further refusals of the argument checks: no levels, sharp entries that are not finite, the residual's entry too
    fr = frames[True, True]
    for levels, sharp, what in ((0, [1.0] * 9, "0 levels"), (-1, [1.0] * 9, "-1 levels"), (2, [np.nan, 1, 1], "sharp[0]"),
                                (2, [1, np.inf, 1], "sharp[1]"), (2, [1, 1, 0.999], "sharp[2]"), (2, [1, -4.0, 1], "sharp[1]")):
        b = capi.BandsStruct()
        b.levels = levels
        for l, s in enumerate(sharp):
            b.sharp[l] = s
        out = np.zeros((H, W, 3), np.uint8)
        assert fr._L.vm_frame_render_multiband(fr._h, C.byref(b), 0.3, 0.35, out.ctypes.data, 0) == INV
        assert what in fr._L.vm_last_error().decode()
    # entries past sharp[levels] are not read
    b = Bands.linear(2).struct()
    b.sharp[3] = np.nan
    assert fr._L.vm_frame_render_multiband(fr._h, C.byref(b), 0.3, 0.35, out.ctypes.data, 0) == OK
    for k, fr in frames.items():
        for i, (a, c) in enumerate(zip(before[k], _state(fr, *k))):
            assert _same(a, c), (k, i)


def test_two_faults_at_once_answer_in_the_render_calls_order(frames):
    before = {k: fr.render_halfway(0.3, 0.35, 1) for k, fr in frames.items()}
    checked = 0
    for name in CALLS:
        for pair in itertools.combinations(_expressible(name), 2):
            if sum(f in BANDS_FAULTS for f in pair) == 2 or ("null_bands" in pair and "sharp" in pair):
                continue                    # one vm_bands cannot carry both
            for dev in (False, True):
                mine = [f for f in pair if not (dev and f in ("null_output", "pitch"))]
                rc, msg = _call(frames, name, mine, dev)
                what = (name, pair, dev, msg)
                checked += 1
                if not mine:
                    assert rc == OK, what
                    continue
                first = min(mine, key=lambda f: FAULTS[f][0])
                assert rc == FAULTS[first][1], what
                assert msg.startswith(name + ("_dev: " if dev else ": ")) and FAULTS[first][2] in msg, what
    # pairs of 6, 7, 8 and 9 faults, less the four that one vm_bands cannot carry, on the call and on its twin
    assert checked == 2 * ((15 - 4) + (21 - 4) + (28 - 4) + (36 - 4))
    for k, fr in frames.items():
        assert np.array_equal(fr.render_halfway(0.3, 0.35, 1), before[k]), k


def test_pitched_outputs_and_times(frames):
    """a pitch above the row keeps what lies beyond the rows; the _dev twins give a positive time, or none if not asked"""
    fr = frames[True, True]
    bands = Bands.sharpen(2, 4)
    b = bands.struct()
    big = np.full((H, 3 * W + 5), 201, np.uint8)
    capi.check(fr._L.vm_frame_render_multiband(fr._h, C.byref(b), 0.3, 0.35, big.ctypes.data, 3 * W + 5))
    assert np.array_equal(big[:, :3 * W].reshape(H, W, 3), fr.render_multiband(bands, 0.3, 0.35)) and np.all(big[:, 3 * W:] == 201)
    bigf = np.full((H, CH * W + 3), np.float32(-12345.5), np.float32)
    capi.check(fr._L.vm_frame_render_multiband_transition_layers(fr._h, C.byref(b), 0.4, capi.EASE_SMOOTH, bigf.ctypes.data, CH * W + 3))
    assert _same(bigf[:, :CH * W].reshape(H, W, CH), fr.render_multiband_transition_layers(bands, 0.4, capi.EASE_SMOOTH))
    assert np.all(bigf[:, CH * W:] == np.float32(-12345.5))
    assert fr.render_multiband_dev(bands, 0.3, 0.35) > 0 and fr.render_multiband_transition_layers_dev(bands, 0.4) > 0
    capi.check(fr._L.vm_frame_render_multiband_layers_dev(fr._h, C.byref(b), 0.3, 0.35, None))
