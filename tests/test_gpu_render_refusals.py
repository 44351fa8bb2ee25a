"""The one order in which the render calls refuse (include/vmorph.h), on all 28 of them: after the handle
guard a NULL output (a call that downloads), the arguments (viewport, samples, ease, color_from), the frame's state (no
schedule, then no layers), the pitch.  A call that carries two faults at once answers with the code -- and the message --
of the earlier one, and so does its _dev twin, which cannot carry a NULL output or a pitch and answers for what is left
of the pair.  Every call here is refused by a check on the host, or is a good call.

The frames are 33 x 7 with ex = 3, as in the refusal tests of the families: instant, and no row pitch is a multiple of
anything convenient.  Four of them, with and without a schedule and layers: a fault of the frame's state is the choice of
the frame."""
import ctypes as C
import itertools

import numpy as np
import pytest

import warp_ref
from videomorphing_amd import capi, morph, synth, transition
from videomorphing_amd.viewport import Viewport

pytestmark = pytest.mark.gpu

W, H, EX, CH = 33, 7, 3, 2
OK, ST, INV = capi.VM_OK, capi.VM_E_STATE, capi.VM_E_INVALID
GOOD_VP = Viewport(2.25, 0.5, 0.8, 0.8, 21, 6, 2, 2)
UNIFORM = dict(color_fa=0.3, geo_fa=0.35, color_from=1)
SCHEDULED = dict(t=0.4, ease=capi.EASE_LINEAR, color_from=1)
SHUTTER = dict(color_fa=0.3, geo_open=0.4, geo_close=0.6, samples=4, color_from=1)
TSHUTTER = dict(t_open=0.4, t_close=0.6, samples=4, t_color=0.5, ease=capi.EASE_SMOOTH, color_from=1)
# the calls that download and a good argument tuple of each, in the C order; every one has a _dev twin with the same
# arguments: 28 entry points.  A call takes a viewport, a sample count or an ease where its arguments name one, needs a
# schedule where it takes an ease, and needs layers where its name says so.
CALLS = [
    ("vm_render_halfway", UNIFORM),
    ("vm_render_layers", UNIFORM),
    ("vm_render_transition", SCHEDULED),
    ("vm_render_transition_layers", SCHEDULED),
    ("vm_render_shutter", SHUTTER),
    ("vm_render_shutter_layers", SHUTTER),
    ("vm_render_transition_shutter", TSHUTTER),
    ("vm_render_transition_shutter_layers", TSHUTTER),
    ("vm_render_viewport", dict(vp=GOOD_VP, **UNIFORM)),
    ("vm_render_viewport_layers", dict(vp=GOOD_VP, **UNIFORM)),
    ("vm_render_viewport_shutter", dict(vp=GOOD_VP, **SHUTTER)),
    ("vm_render_viewport_shutter_layers", dict(vp=GOOD_VP, **SHUTTER)),
    ("vm_render_viewport_transition_shutter", dict(vp=GOOD_VP, **TSHUTTER)),
    ("vm_render_viewport_transition_shutter_layers", dict(vp=GOOD_VP, **TSHUTTER)),
]
# fault -> (its place in the order, the code, what the message says); the first two are the downloading call's alone
FAULTS = {
    "null_output": (0, INV, "output is NULL"),
    "pitch": (7, INV, "below the row"),
    "null_viewport": (1, INV, "viewport is NULL"),
    "samples": (2, INV, "0 samples"),
    "ease": (3, INV, "ease 2"),
    "color_from": (4, INV, "color_from 3"),
    "no_schedule": (5, ST, "holds no schedule"),
    "no_layers": (6, ST, "holds no layers"),
}
STEP = {"null_output": 2, "null_viewport": 3, "samples": 3, "ease": 3, "color_from": 3, "no_schedule": 4, "no_layers": 4, "pitch": 5}


def _expressible(name, args):
    """the faults the downloading call `name` can carry"""
    out = ["null_output", "pitch", "color_from"]
    out += [f for f, key in (("null_viewport", "vp"), ("samples", "samples"), ("ease", "ease"), ("no_schedule", "ease")) if key in args]
    return out + (["no_layers"] if name.endswith("_layers") else [])


def test_the_table_is_every_render_entry_point():
    names = [n for n, _ in CALLS] + [n + "_dev" for n, _ in CALLS]
    assert len(set(names)) == 28 and sorted(names) == sorted(n for n in capi.SYMBOLS if n.startswith("vm_render_"))


def test_two_faults_at_once_answer_in_one_order(gpu_ctx):
    rng = np.random.RandomState(7)
    v = warp_ref.field("smooth", W, H, rng)
    u = warp_ref.path(W, H, rng)
    rgb0, rgb1 = synth.make_rgb_pair(W, H)
    layers = [rng.randn(H, W, CH).astype(np.float32) for _ in range(2)]
    frames = {}
    for sched, lay in itertools.product((False, True), repeat=2):
        fr = morph.Frame(gpu_ctx, W, H, EX)
        fr.upload(morph.make_extended(rgb0, EX), morph.make_extended(rgb1, EX), v, u)
        if sched:
            fr.upload_schedule(transition.wipe(W, H), transition.radial(W, H))
        if lay:
            fr.upload_layers(*layers)
        frames[sched, lay] = fr
    L = capi.load()
    before = {k: fr.render_halfway(0.3, 0.35, 1) for k, fr in frames.items()}
    host = np.zeros(64 * 64 * 4, np.float32)
    ms = C.c_float(0)
    gs = GOOD_VP.struct()

    def call(name, args, faults, dev):
        """(code, message) of `name` (dev: of its twin) with its good arguments and the given faults"""
        fr = frames["no_schedule" not in faults, "no_layers" not in faults]
        a = dict(args)
        if "vp" in a:
            a["vp"] = None if "null_viewport" in faults else C.byref(gs)
        for fault, key, bad in (("samples", "samples", 0), ("ease", "ease", 2), ("color_from", "color_from", 3)):
            if fault in faults:
                a[key] = bad
        if dev:
            rc = getattr(L, name + "_dev")(fr._h, *a.values(), C.byref(ms))
        else:
            row = (GOOD_VP.out_w if "vp" in a else W) * (CH if name.endswith("_layers") else 3)
            rc = getattr(L, name)(fr._h, *a.values(), None if "null_output" in faults else host.ctypes.data,
                                  row - 1 if "pitch" in faults else 0)
        return rc, L.vm_last_error().decode()

    checked = 0
    for name, args in CALLS:
        can = _expressible(name, args)
        assert call(name, args, (), False)[0] == OK and call(name, args, (), True)[0] == OK, name
        for pair in itertools.combinations(can, 2):
            for dev in (False, True):
                # the twin answers for the faults it can carry; with none left it is a good call
                mine = [f for f in pair if not (dev and f in ("null_output", "pitch"))]
                rc, msg = call(name, args, mine, dev)
                what = (name, pair, dev, msg)
                checked += STEP[pair[0]] != STEP[pair[1]]
                if not mine:
                    assert rc == OK, what
                    continue
                first = min(mine, key=lambda f: FAULTS[f][0])
                assert rc == FAULTS[first][1], what
                assert msg.startswith(name + ("_dev: " if dev else ": ")) and FAULTS[first][2] in msg, what
    # every pair of faults from two different steps of the order (pairs within a step are held as well), per call of the
    # table in its order, on the call and on its twin
    assert checked == 2 * (3 + 6 + 9 + 13 + 5 + 9 + 12 + 17 + 5 + 9 + 7 + 12 + 15 + 21)
    # a refused call leaves the frame and warp_out usable: every call is still good, the frames render what they rendered
    for name, args in CALLS:
        assert call(name, args, (), False)[0] == OK and call(name, args, (), True)[0] == OK, name
    for k, fr in frames.items():
        assert np.array_equal(fr.render_halfway(0.3, 0.35, 1), before[k]), k
        fr.close()
