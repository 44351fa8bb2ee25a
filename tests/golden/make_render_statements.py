"""Records tests/golden/render_statements.json: what the render tests' float32 numpy statements (tests/warp_ref.py,
transit_ref, shutter_ref, transit_shutter_ref, viewport_ref, vshutter_ref, filter_ref, carry_ref, the render tail of
layer_ext_ref and the plates of multiband_ref) give on fixed small inputs.  No GPU and no library call: numpy only.  It
is recorded BEFORE a change of how those statements are written and must run unchanged after it, so it goes through the
family modules' public functions only; tests/test_render_statements.py holds the current modules to it.

    python3 tests/golden/make_render_statements.py <out.json> [--calls]

Every call gets one sha256 under a readable key.  A float32 array is hashed as its bits with every NaN replaced by one
pattern first (what render_cases.same_bits compares: a NaN for a NaN); dtype and shape are hashed with it.  A key that
ends in "cf*" or "c*" holds the call under every color_from or every channel count, hashed in turn.  The file keeps one
sha256 per GROUP of calls -- a family's calls on one shape and one field, their keys and hashes in call order -- so that
it stays a few kilobytes; --calls writes the hash of every call instead, to find the call that moved: record both sides
of a change that way and compare."""
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import carry_ref  # noqa: E402
import filter_ref  # noqa: E402
import layer_ext_ref  # noqa: E402
import multiband_ref  # noqa: E402
import shutter_ref  # noqa: E402
import transit_ref  # noqa: E402
import transit_shutter_ref as TS  # noqa: E402
import viewport_ref  # noqa: E402
import vshutter_ref as VS  # noqa: E402
import warp_ref  # noqa: E402
from render_cases import field, layers  # noqa: E402
from videomorphing_amd import transition  # noqa: E402

f32 = np.float32
ONE_NAN = np.uint32(0x7FC00000)
SHAPES = [(33, 7, 3), (5, 3, 2), (45, 27, 4)]                   # (w, h, ex)
# (kind of warp_ref.field, with a path): every kind, the smooth and the nan one both ways
FIELDS = [("smooth", False), ("smooth", True), ("large", True), ("outside", False), ("nan", False), ("nan", True)]
SHUTTERS = [(0.3, 0.7), (0.7, 0.3), (-0.2, 0.2)]
SAMPLES = [1, 2, 5]
PAIRED = list(zip(SHUTTERS, (2, 5, 1))) + [((0.3, 0.7), 5)]     # the families with many chains a sample take these
CFS = (0, 1, 2)
CHANNELS = [1, 3, 4]
FILTERS = [filter_ref.BILINEAR, filter_ref.CATMULL_ROM, filter_ref.MITCHELL, filter_ref.BSPLINE]
SHARP = {5: [1.0, 2.0], 33: [1.0, 1.5, 2.0], 45: [1.0, 1.25, 1.5, 3.0]}      # by width: as many levels as the shape bears


def digest(arrays):
    """(sha256 of the arrays' dtypes, shapes and bits, the number of NaNs among them)"""
    sha, nans = hashlib.sha256(), 0
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.uint8, np.bool_, np.int64), a.dtype
        sha.update(("%s%r" % (a.dtype, a.shape)).encode())
        if a.dtype == np.float32:
            bits = a.view(np.uint32).copy()
            isnan = np.isnan(a)
            bits[isnan] = ONE_NAN
            nans += int(isnan.sum())
            a = bits
        sha.update(a.tobytes())
    return sha.hexdigest(), nans


def flat(x):
    """the arrays of a result: an array, or tuples and lists of them to any depth"""
    if isinstance(x, (tuple, list)):
        return [a for t in x for a in flat(t)]
    return [np.asarray(x)]


def canvases(w, h, ex):
    rng = np.random.RandomState(5)
    return [rng.randint(0, 256, (h + 2 * ex, w + 2 * ex, 4)).astype(np.uint8) for _ in range(2)]


def schedules(w, h):
    """name -> (geometry, colour): none, a wipe under a radial colour plane, random pairs with steps (t1 <= t0)"""
    rng = np.random.RandomState(23)
    pairs = []
    for _ in range(2):
        s = rng.rand(h, w, 2).astype(f32)
        s[..., 1] += f32(0.2)
        s[rng.rand(h, w) < 0.3, 1] = f32(0.1)
        pairs.append(s)
    return {"none": (None, None), "wipe": (transition.wipe(w, h), transition.radial(w, h)), "pairs": tuple(pairs)}


def viewports(w, h):
    out = {"identity": (0.0, 0.0, 1.0, 1.0, w, h, 1, 1), "zoom": (1.25, 0.5, 0.4, 0.4, 12, 7, 2, 2)}
    for i, vp in enumerate(viewport_ref.EDGE_VIEWPORTS):
        out["edge%d" % i] = vp
    return out


def entries():
    """(key, result) of every call, in a fixed order"""
    for filt in FILTERS[1:]:
        yield "filter.weights/f%d" % filt, filter_ref.weights(np.linspace(0, 1, 33, endpoint=False).astype(f32), filt)
    for n in (1, 2, 3, 8, 64):
        yield "viewport.sample_fractions/%d" % n, viewport_ref.sample_fractions(n)
    for (o, c) in SHUTTERS:
        for n in SAMPLES + [64]:
            yield "shutter.sample_times/%r/%d" % ((o, c), n), shutter_ref.sample_times(o, c, n)
            yield "tshutter.sample_times/%r/%d" % ((o, c), n), TS.sample_times(o, c, n)
    for w, h, ex in SHAPES:
        shape = "%dx%d" % (w, h)
        e0, e1 = canvases(w, h, ex)
        lay = [(layers(w, h, c, 1), layers(w, h, c, 2)) for c in CHANNELS]
        lay_ext = [(layers(w + 2 * ex, h + 2 * ex, c, 3), layers(w + 2 * ex, h + 2 * ex, c, 4)) for c in CHANNELS]
        scheds = schedules(w, h)
        vps = viewports(w, h)
        yield shape + "/transit.uniform_schedule", transit_ref.uniform_schedule(w, h)
        yield shape + "/transit.two_halves", transit_ref.two_halves(w, h)
        yield shape + "/carry.grid", carry_ref.grid(w, h)
        for name in ("wipe", "pairs"):
            for ease in (0, 1):
                yield "%s/transit.ramp/%s/e%d" % (shape, name, ease), [transit_ref.ramp(scheds[name][0], t, ease) for t in (-0.5, 0.0, 0.45, 1.0, 1.5)]
        for name, vp in vps.items():
            yield "%s/viewport.sample_points/%s" % (shape, name), viewport_ref.sample_points(vp)
        rgb, v0, vp0 = filter_ref.overshoot_case(w, h)
        yield shape + "/filter.overshoot_case", (rgb, v0, np.asarray(vp0[:4], f32), np.asarray(vp0[4:], np.int64))
        rng = np.random.RandomState(77)
        pts = np.stack([rng.uniform(-3, w + 3, 40), rng.uniform(-3, h + 3, 40)], -1).astype(f32)
        cons = np.concatenate([pts[:12], pts[12:24], np.ones((12, 1), f32)], -1)
        for kind, with_path in FIELDS:
            v, u = field(w, h, kind, with_path)
            for key, res in family_entries(w, h, ex, v, u, e0, e1, lay, lay_ext, scheds, vps, pts, cons):
                yield "%s/%s/%s/%s" % (shape, kind, "path" if with_path else "nopath", key), res


def family_entries(w, h, ex, v, u, e0, e1, lay, lay_ext, scheds, vps, pts, cons):
    # ---- warp_ref, and the render tail of layer_ext_ref
    for geo in (0.0, 0.3, 1.0):
        yield "warp.sampling_maps/%r" % geo, warp_ref.sampling_maps(v, u, geo)
    map0, map1 = warp_ref.sampling_maps(v, u, 0.3)[:2]
    yield "warp.inside_flags", warp_ref.inside_flags(map0, map1)
    yield "warp.render_bytes/cf*", [warp_ref.render_bytes(e0, e1, ex, map0, map1, 0.6, cf) for cf in CFS]
    for cf in CFS:
        yield "warp.render_layers/cf%d/c*" % cf, [warp_ref.render_layers(l0, l1, map0, map1, 0.6, cf) for l0, l1 in lay]
        yield "layer_ext.render_layers/cf%d/c*" % cf, [layer_ext_ref.render_layers(l0, l1, ex, map0, map1, 0.6, cf) for l0, l1 in lay_ext]
    # ---- multiband_ref's plates and the calls on them
    sharp = SHARP[w]
    uni = multiband_ref.uniform_inputs(v, u, 0.6, 0.3)
    yield "multiband.uniform_inputs", uni
    yield "multiband.canvas_plates", multiband_ref.canvas_plates(e0, e1, ex, map0, map1)
    yield "multiband.render_bytes/uniform", multiband_ref.render_bytes(e0, e1, ex, uni, sharp)
    yield "multiband.layer_plates/lex0/c*", [multiband_ref.layer_plates(l0, l1, map0, map1) for l0, l1 in lay]
    yield "multiband.layer_plates/lex/c*", [multiband_ref.layer_plates(l0, l1, map0, map1, ex) for l0, l1 in lay_ext]
    yield "multiband.render_layers/lex0/c*", [multiband_ref.render_layers(l0, l1, uni, sharp) for l0, l1 in lay]
    yield "multiband.render_layers/lex/c*", [multiband_ref.render_layers(l0, l1, uni, sharp, ex) for l0, l1 in lay_ext]
    # ---- transit_ref
    for name, (sg, sc) in scheds.items():
        for ease in (0, 1):
            tag = "%s/e%d" % (name, ease)
            tm = transit_ref.transition_maps(v, u, sg, sc, 0.45, ease)
            k = tm[4][..., 1]
            yield "transit.transition_maps/" + tag, tm
            yield "transit.render_bytes/%s/cf*" % tag, [transit_ref.render_bytes(e0, e1, ex, tm[0], tm[1], k, cf) for cf in CFS]
            yield "transit.render_layers/%s/cf*/c*" % tag, [transit_ref.render_layers(l0, l1, tm[0], tm[1], k, cf) for cf in CFS for l0, l1 in lay]
            sched_in = multiband_ref.scheduled_inputs(v, u, sg, sc, 0.45, ease)
            yield "multiband.scheduled_inputs/" + tag, sched_in
            yield "multiband.render_bytes/" + tag, multiband_ref.render_bytes(e0, e1, ex, sched_in, sharp)
    yield "transit.two_halves_columns", transit_ref.two_halves_columns(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0), w)
    # ---- shutter_ref, and the sample loops' tail of layer_ext_ref
    for (o, cl) in SHUTTERS:
        for n in SAMPLES:
            tag = "%r/%d" % ((o, cl), n)
            maps = shutter_ref.sample_maps(v, u, o, cl, n)
            yield "shutter.sample_maps/" + tag, maps
            yield "shutter.canvas_mean/%s/cf*" % tag, [shutter_ref.canvas_mean(e0, e1, ex, maps, 0.6, cf) for cf in CFS]
            yield "shutter.layers_on_maps/%s/c*" % tag, [shutter_ref.layers_on_maps(l0, l1, maps, 0.6, 1) for l0, l1 in lay]
            yield "layer_ext.layers_on_maps/%s/c*" % tag, [layer_ext_ref.layers_on_maps(l0, l1, ex, maps, 0.6, 1) for l0, l1 in lay_ext]
        yield "shutter.render_shutter_bytes/%r" % ((o, cl),), shutter_ref.render_shutter_bytes(e0, e1, ex, v, u, 0.6, o, cl, 2, 1)
        yield "shutter.render_shutter_layers/%r" % ((o, cl),), shutter_ref.render_shutter_layers(lay[1][0], lay[1][1], v, u, 0.6, o, cl, 2, 1)
    # ---- transit_shutter_ref
    for name, ease in (("none", 0), ("wipe", 0), ("wipe", 1), ("pairs", 1)):
        sg, sc = scheds[name]
        for (o, cl), n in (PAIRED if name != "none" else PAIRED[:1]):
            tag = "%s/e%d/%r/%d" % (name, ease, (o, cl), n)
            maps = TS.sample_maps(v, u, sg, sc, o, cl, n, 0.45, ease)
            yield "tshutter.sample_maps/" + tag, maps
            yield "tshutter.canvas_mean/%s/cf*" % tag, [TS.canvas_mean(e0, e1, ex, maps, cf) for cf in CFS]
            yield "tshutter.layers_on_maps/%s/c*" % tag, [TS.layers_on_maps(l0, l1, maps, 1) for l0, l1 in lay]
        yield "tshutter.render_layers/%s/e%d" % (name, ease), TS.render_layers(lay[1][0], lay[1][1], v, u, sg, sc, 0.3, 0.7, 2, 0.45, ease, 1)
    sg, sc = scheds["pairs"]
    yield "tshutter.walk", TS.walk(v, u, transit_ref.ramp(sg, 0.4, 1), transit_ref.ramp(sc, 0.6, 0))
    # ---- viewport_ref, and filter_ref on its maps
    for name, vp in vps.items():
        maps = viewport_ref.sample_maps(v, u, 0.3, vp)
        yield "viewport.sample_maps/" + name, maps
        yield "viewport.render_viewport_bytes/%s/cf*" % name, [viewport_ref.render_viewport_bytes(e0, e1, ex, v, u, 0.6, 0.3, cf, vp, maps) for cf in CFS]
        yield "viewport.layers_on_maps/%s/c*" % name, [viewport_ref.layers_on_maps(l0, l1, maps, 0.6, 1) for l0, l1 in lay]
        if name not in ("identity", "zoom"):
            continue
        yield "viewport.render_viewport_bytes/%s/its own maps" % name, viewport_ref.render_viewport_bytes(e0, e1, ex, v, u, 0.6, 0.3, 1, vp)
        yield "viewport.render_viewport_layers/" + name, viewport_ref.render_viewport_layers(lay[1][0], lay[1][1], v, u, 0.6, 0.3, 1, vp)
        for filt in (FILTERS if name == "zoom" else FILTERS[:2]):
            tag = "%s/f%d" % (name, filt)
            taps = filter_ref.canvas_taps(e0, e1, ex, maps, filt)
            yield "filter.canvas_taps/" + tag, taps
            yield "filter.canvas_mean/" + tag, filter_ref.canvas_mean(e0, e1, ex, maps, 0.6, 1, filt)
            yield "filter.render_viewport_bytes/%s/cf*" % tag, [filter_ref.render_viewport_bytes(e0, e1, ex, maps, 0.6, cf, filt, taps) for cf in CFS]
            yield "filter.layer_taps/%s/lex0/c*" % tag, [filter_ref.layer_taps(l0, l1, maps, filt) for l0, l1 in lay]
            yield "filter.layer_taps/%s/lex/c*" % tag, [filter_ref.layer_taps(l0, l1, maps, filt, ex) for l0, l1 in lay_ext]
            yield "filter.layers_on_maps/%s/lex0/c*" % tag, [filter_ref.layers_on_maps(l0, l1, maps, 0.6, 1, filt) for l0, l1 in lay]
            yield "filter.layers_on_maps/%s/lex/c*" % tag, [filter_ref.layers_on_maps(l0, l1, maps, 0.6, 1, filt, ex) for l0, l1 in lay_ext]
    qx, qy = viewport_ref.sample_points(vps["zoom"])[1]
    yield "viewport.landing", viewport_ref.landing(v, u, 0.7, qx, qy)
    with np.errstate(all="ignore"):
        x, y = map0[..., 0] + f32(ex + 0.5), map0[..., 1] + f32(ex + 0.5)
        yield "filter.tap/f*", [filter_ref.tap(e0[..., :3].astype(f32), x, y, filt) for filt in FILTERS]
    # ---- vshutter_ref
    for name, vp in vps.items():
        for (o, cl), n in (PAIRED if name == "zoom" else [((0.3, 0.7), 2 if name == "identity" else 1)]):
            tag = "%s/%r/%d" % (name, (o, cl), n)
            maps = VS.uniform_maps(v, u, o, cl, n, vp)
            yield "vshutter.uniform_maps/" + tag, maps
            yield "vshutter.bytes_on_maps/%s/cf*" % tag, [VS.bytes_on_maps(e0, e1, ex, maps, cf, 0.6) for cf in CFS]
            yield "vshutter.layers_on_maps/%s/c*" % tag, [VS.layers_on_maps(l0, l1, maps, 1, 0.6) for l0, l1 in lay]
            for sname, ease in {"zoom": (("wipe", 1), ("pairs", 0)), "identity": (("wipe", 1),), "edge2": (("wipe", 1),)}.get(name, ()):
                sg, sc = scheds[sname]
                maps = VS.scheduled_maps(v, u, sg, sc, o, cl, n, 0.45, ease, vp)
                yield "vshutter.scheduled_maps/%s/%s" % (tag, sname), maps
                yield "vshutter.bytes_on_maps/%s/%s/cf*" % (tag, sname), [VS.bytes_on_maps(e0, e1, ex, maps, cf) for cf in CFS]
                yield "vshutter.layers_on_maps/%s/%s/c*" % (tag, sname), [VS.layers_on_maps(l0, l1, maps, 1) for l0, l1 in lay]
    vp, (sg, sc) = vps["zoom"], scheds["wipe"]
    yield "vshutter.render_viewport_shutter_bytes", VS.render_viewport_shutter_bytes(e0, e1, ex, v, u, 0.6, 0.3, 0.7, 2, 1, vp)
    yield "vshutter.render_viewport_transition_shutter_layers", VS.render_viewport_transition_shutter_layers(
        lay[1][0], lay[1][1], v, u, sg, sc, 0.3, 0.7, 2, 0.45, 1, 1, vp)
    # ---- carry_ref: from off-grid points and from the grid
    for where, q in (("points", pts), ("grid", carry_ref.grid(w, h))):
        for t_from in (0.0, 0.3, 1.0):
            yield "carry.carry/%s/%r" % (where, t_from), carry_ref.carry(v, u, q, t_from, [0.0, 0.25, 1.0, 1.5])
        for name, (sg, _) in scheds.items():
            for ease in (0, 1):
                yield "carry.carry_transition/%s/%s/e%d" % (where, name, ease), carry_ref.carry_transition(v, u, sg, q, 0.45, [0.0, 0.6, 1.0], ease)
    yield "carry.constraint_gaps", carry_ref.constraint_gaps(v, u, cons)
    yield "carry.constraint_gaps/no rows", carry_ref.constraint_gaps(v, u, np.empty((0, 5), f32))


def record():
    """{key: sha256}, and the number of NaNs hashed under the keys of the `nan` field"""
    out, nans = {}, 0
    for key, res in entries():
        assert key not in out, key
        out[key], n = digest(flat(res))
        if "/nan/" in key:
            nans += n
    return out, nans


def group_of(key):
    """"33x7/nan/path/shutter.canvas_mean/(0.3, 0.7)/2/cf*" -> "33x7/nan/path/shutter": the key up to the function's
    name, and of that name the family"""
    parts = key.split("/")
    at = next(i for i, p in enumerate(parts) if re.match(r"[a-z_]+\.[a-z_]+$", p))
    return "/".join(parts[:at] + [parts[at].split(".")[0]])


def groups(calls):
    """{group: [the number of its calls, sha256 of their keys and hashes in call order]}"""
    shas = {}
    for key, sha in calls.items():                  # a dict keeps the order of the calls
        shas.setdefault(group_of(key), []).append("%s %s\n" % (key, sha))
    return {g: [len(lines), hashlib.sha256("".join(lines).encode()).hexdigest()] for g, lines in shas.items()}


def main():
    calls, nans = record()
    assert nans > 0
    out = calls if "--calls" in sys.argv[2:] else groups(calls)
    with open(sys.argv[1], "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(out[k])) for k in sorted(out)) + "\n}\n")
    print(len(calls), "calls in", len(groups(calls)), "groups,", nans, "NaNs under the nan field")


if __name__ == "__main__":
    main()
