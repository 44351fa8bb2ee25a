"""Inputs of the temporal path's stage tests: level shapes and flow / field cases, each built to show one
edge of the forward splat, its normalisation, the 3x3 smoothing and the row fill.

A case is a function of (w, h, seed) that returns a dict of float32 arrays

    v        two fields (h, w, 2): of the page before and of the page after the page under test
    f0, f1   the forward flows of the page before  (temp_ref taps f0 at p - v and f1 at p + v)
    b0, b1   the backward flows of the page after

so that initialize_temp(dir = -1) reads (v[0], f0, f1), initialize_temp(dir = +1) reads (v[1], b0, b1)
and the in-between page of upsample() reads both.  tests/test_temporal_ref.py asserts on the oracle's
result alone that every case shows, at every shape, what it was built to show; the figures it prints
(hole share, largest collision count, largest accumulated weight) are in the docstring of
tests/test_gpu_temporal_stages.py.

NaN and infinite flows are out of scope: (int)floorf and llrint of a NaN are undefined in the
reference, in the oracle and on the device."""
import numpy as np

from videomorphing_amd import synth

F32 = np.float32

# (w, h).  vm_video_create needs at least 5 x 5; a workgroup of the temporal kernels is 64 x 4 pixels.
SHAPES = [
    (5, 5),        # minimum size
    (5, 70),       # a single column of work, many 4-row workgroups
    (70, 5),       # two workgroup columns, two rows of workgroups
    (63, 8), (64, 8), (65, 9),   # either side of the 64-wide workgroup
    (129, 7),      # three workgroup columns
    (33, 37),      # row pitch 64 > w: the padding must never be read as a pixel
    (257, 131),    # mid size: targets reached from other workgroups in both directions
]


def smooth_flow(rng, w, h, amp):
    """the gentle sinusoidal flow of tests/test_gpu_temporal.py"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a, b, c, d = rng.rand(4) * 2 * np.pi
    fx = amp * np.sin(2 * np.pi * x / w + a) * np.cos(2 * np.pi * y / h + b) + 0.3 * amp
    fy = amp * np.cos(2 * np.pi * x / w + c) * np.sin(2 * np.pi * y / h + d) - 0.2 * amp
    return np.stack([fx, fy], -1).astype(np.float32)


def _grid_v(rng, w, h, amp=1.5):
    """random vectors on the 2^-16 grid: their products with a weight of 1 and their sums of two are
    exact in the 2^-32 fixed point"""
    return (np.rint(rng.randn(h, w, 2) * amp * 65536) / 65536).astype(F32)


def _const(w, h, fx, fy):
    f = np.empty((h, w, 2), F32)
    f[..., 0], f[..., 1] = fx, fy
    return f


def _pack(v, f0, f1, b0, b1):
    return dict(v=[np.ascontiguousarray(a, dtype=F32) for a in v],
                **{k: np.ascontiguousarray(a, dtype=F32) for k, a in (("f0", f0), ("f1", f1), ("b0", b0), ("b1", b1))})


def zero(w, h, seed):
    """zero flows, random v: every pixel lands on itself with weight exactly 1 and adds three
    contributions of weight exactly 0 to its neighbours"""
    rng = np.random.RandomState(seed)
    z = np.zeros((h, w, 2), F32)
    return _pack([_grid_v(rng, w, h), _grid_v(rng, w, h)], z, z, z, z)


SHIFT = (3, -2)


def shift(w, h, seed):
    """the whole-number flow (+3, -2) on both videos and in both directions: whole-number landing
    positions; columns 0..2 and rows h-2, h-1 receive nothing.  v lies on the 1/4 grid: the bilinear
    weights of the two taps are then multiples of 1/16 and each tap returns the constant exactly (at any
    other v the four-term sum rounds, and the landing position is a whole number only nearly)."""
    rng = np.random.RandomState(seed)
    f = _const(w, h, *SHIFT)
    v = [(np.rint(rng.randn(h, w, 2) * 6) / 4).astype(F32) for _ in range(2)]
    return _pack(v, f, f, f, f)


def gaps_split(w):
    """(column of the line, whole-number shift away from it)"""
    return w // 2, (1 if w < 16 else 3)


def gaps(w, h, seed):
    """whole-number flows that part at a vertical line (-s left of it, +s right of it) with whole-number
    v in {-1, 0, 1}: whole-number landing positions, an interior gap up to 2 s wide whose pixels have
    weighted neighbours at unequal distances on both sides"""
    rng = np.random.RandomState(seed)
    x0, s = gaps_split(w)
    f = np.zeros((h, w, 2), F32)
    f[:, :x0, 0], f[:, x0:, 0] = -s, s
    v = [rng.randint(-1, 2, size=(h, w, 2)).astype(F32) for _ in range(2)]
    if w < 16:      # a tap across the line would close a gap of two pixels
        for a in v:
            a[..., 0] = 0
    return _pack(v, f, f, f, f)


def converge(w, h, seed):
    """flows that carry every pixel to one point next to the frame centre: w h contributions per launch
    on at most 9 targets, nothing anywhere else"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    cx, cy = F32(w // 2 - 0.375), F32(h // 2 - 0.375)     # a fractional point: four targets share the weight
    f = np.stack([cx - x, cy - y], -1).astype(F32)
    v = [(rng.rand(h, w, 2) - 0.5).astype(F32) for _ in range(2)]    # |v| <= 0.5: clamped taps move a landing by < 0.5
    return _pack(v, f, f, f, f)


def leave(w, h, seed):
    """every pixel leaves the frame"""
    rng = np.random.RandomState(seed)
    fa, fb = _const(w, h, 2 * w + 3.25, 0.5), _const(w, h, -0.25, -(2 * h + 1.75))
    return _pack([_grid_v(rng, w, h), _grid_v(rng, w, h)], fa, fa, fb, fb)


def rim(w, h, seed):
    """landing positions on the lines x = -1, x = w - 1, y = -1, y = h - 1 and a fraction (0, 1/4, 1/2, 3/4)
    inside them, one line per pixel in turn: only the in-frame part of each footprint is added.  v = 0, so the
    flows are read at the pixel itself; f1 - f0 = 2 e gives the advected vector e."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    g = (x + 2 * y + seed) % 4
    frac = rng.randint(0, 4, size=(h, w)) / 4.0
    tx = np.where(g == 0, -1 + frac, np.where(g == 1, w - 1 + frac, x))
    ty = np.where(g == 2, -1 + frac, np.where(g == 3, h - 1 + frac, y))
    d = np.stack([tx - x, ty - y], -1)                                  # multiples of 1/4: exact
    out = []
    for _ in range(2):
        e = rng.randint(-16, 17, size=(h, w, 2)) / 8.0
        out += [(d - e).astype(F32), (d + e).astype(F32)]
    z = np.zeros((h, w, 2), F32)
    return _pack([z, z], *out)


def far(w, h, seed):
    """|v| up to 1.5 times the frame with smooth flows: the two taps at p -/+ v clamp on every side"""
    rng = np.random.RandomState(seed)
    v = [((rng.rand(h, w, 2) * 2 - 1) * 1.5 * np.float32([w, h])).astype(F32) for _ in range(2)]
    fl = [smooth_flow(rng, w, h, 1.2) for _ in range(4)]
    return _pack(v, *fl)


def noise_amp(w, h):
    """+/- 8 px, less on frames a flow of 8 px would empty"""
    return min(8.0, 0.4 * min(w, h))


def noise(w, h, seed):
    """white-noise flows of +/- 8 px plus a step: the right half is carried a quarter of the width (at least
    2 px) back over the left half (the lower half over the upper one on narrow frames): collisions where the
    halves overlap, holes where the carried half came from and wherever the noise leaves one."""
    rng = np.random.RandomState(seed)
    amp = noise_amp(w, h)
    fl = [((rng.rand(h, w, 2) * 2 - 1) * amp).astype(F32) for _ in range(4)]
    for f in fl:
        if w >= h:
            f[:, w // 2:, 0] -= F32(max(0.25 * w, 2.0))
        else:
            f[h // 2:, :, 1] -= F32(max(0.25 * h, 2.0))
    v = [(rng.randn(h, w, 2) * 1.5).astype(F32) for _ in range(2)]
    return _pack(v, *fl)


def smooth_1(w, h, seed):
    """the baseline of tests/test_gpu_temporal.py: smooth flows of 1.2 px"""
    rng = np.random.RandomState(seed)
    v = [(rng.randn(h, w, 2) * 1.5).astype(F32) for _ in range(2)]
    return _pack(v, *[smooth_flow(rng, w, h, 1.2) for _ in range(4)])


def smooth_4(w, h, seed):
    """smooth flows of 4 px"""
    rng = np.random.RandomState(seed)
    v = [(rng.randn(h, w, 2) * 0.8).astype(F32) for _ in range(2)]
    return _pack(v, *[smooth_flow(rng, w, h, 4.0) for _ in range(4)])


CASES = dict(zero=zero, shift=shift, gaps=gaps, converge=converge, leave=leave, rim=rim, far=far, noise=noise,
             smooth_1=smooth_1, smooth_4=smooth_4)
SEED = 7


def lumas(w, h, seed, noise_sigma=3.0):
    """the two lumas of a page (the ssim factor of initialize_temp is the page's `value` after init_level)"""
    rng = np.random.RandomState(1000 + seed)
    a, b = synth.make_pair(w, h, frame=seed % 5, amp=0.012 * max(w, 40))
    return ((a + noise_sigma * rng.randn(h, w)).astype(F32), (b + noise_sigma * rng.randn(h, w)).astype(F32))


def coarse_shape(w, h):
    return max(5, (w + 1) // 2), max(5, (h + 1) // 2)


# ---- what each case must show, asserted on a result (the oracle's on the CPU, the device's on the GPU) ----

def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def source(c, dr):
    """(v, fa, fb) that initialize_temp(dir) reads"""
    return (c["v"][0], c["f0"], c["f1"]) if dr < 0 else (c["v"][1], c["b0"], c["b1"])


def _moved(a, dx, dy, fill):
    """out[y + dy, x + dx] = a[y, x]"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = a[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def _single_landing(v, value, dx, dy):
    """temp_ref / temp_mask when every pixel lands with weight `value` on the pixel (dx, dy) away and on
    nothing else: mask = value through the 2^-32 grid, ref = (v * value through the grid) / mask.  That is v
    itself to the bit where value == 1; elsewhere v * s / s rounds twice and may miss v by an ulp."""
    import temporal_ref as R
    mask = R.from_fixed(R.to_fixed(value))
    num = R.from_fixed(R.to_fixed((v * value[..., None]).astype(F32)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.where((mask > 0)[..., None], num / mask[..., None], F32(0)).astype(F32)
    return _moved(ref, dx, dy, F32(0)), _moved(np.where(mask > 0, mask, F32(0)).astype(F32), dx, dy, F32(0))


def check_init(name, w, h, c, dr, ref, mask, value):
    """the condition of case `name` on one initialize_temp result (temp_ref and temp_mask were zero before)"""
    import temporal_ref as R
    v = source(c, dr)[0]
    has = mask > 0
    assert not mask[~has].view(np.uint32).any() and not _bits(ref)[~has].any()      # nothing landed: zero bits
    if name in ("zero", "shift"):
        dx, dy = (0, 0) if name == "zero" else SHIFT
        want_ref, want_mask = _single_landing(v, value, dx, dy)
        assert np.array_equal(_bits(mask), _bits(want_mask))
        exact = _moved((value >= 2.0 ** -8) | (value == 0), dx, dy, True)             # on the 2^-32 grid
        assert np.array_equal(_bits(mask)[exact], _bits(_moved(value, dx, dy, F32(0)))[exact])
        assert np.array_equal(_bits(ref), _bits(want_ref))
        one = _moved(value == 1, dx, dy, False)
        assert np.array_equal(_bits(ref)[one], _bits(_moved(v, dx, dy, F32(0)))[one])
        got = np.abs(ref - _moved(v, dx, dy, F32(0)))[has]
        assert (got <= 2.0 ** -23 * np.abs(_moved(v, dx, dy, F32(0)))[has] + 2.0 ** -24).all()
        if name == "shift":                       # the hole strip is exactly those columns and rows
            assert not has[:, :3].any() and not has[h - 2:].any()
            assert np.array_equal(has, _moved(value > 0, dx, dy, False))
    elif name == "gaps":
        left, right = R.nearest_weighted(mask)
        cols = np.broadcast_to(np.arange(w), (h, w))
        two = ~has & (left >= 0) & (right < w)
        assert two.any() and (two & (cols - left != right - cols)).any()
    elif name == "converge":
        assert 1 <= has.sum() <= 9 and has.any(1).sum() <= 3
        assert mask.max() >= 0.2 * value.sum()
    elif name == "leave":
        assert not has.any()
    elif name == "rim":
        assert has[:, 0].any() and has[:, w - 1].any() and has[0].any() and has[h - 1].any()
    elif name == "far":
        y, x = np.mgrid[0:h, 0:w]
        for s in (-1, 1):
            tx, ty = x + s * v[..., 0], y + s * v[..., 1]
            assert (tx < -1).any() and (tx > w).any() and (ty < -1).any() and (ty > h).any()
    elif name == "noise":
        assert 0.05 <= 1 - has.mean() <= 0.60, 1 - has.mean()
    else:
        assert has.mean() > 0.5


def smooth_of_mean(vp, vn):
    """zero flows: the in-between page is the 3x3 mean of float(v_prev + v_next) / 2 (both land with weight 1); the sum
    is taken on the 2^-32 grid, which components below 2^-8 do not lie on"""
    import temporal_ref as R
    h, w = vp.shape[:2]
    m = (R.from_fixed(R.to_fixed(vp) + R.to_fixed(vn)) / F32(2)).astype(F32)
    s, n = np.zeros((h, w, 2), F32), np.zeros((h, w), F32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ok = _moved(np.ones((h, w), bool), -dx, -dy, False)
            s = np.where(ok[..., None], s + _moved(m, -dx, -dy, F32(0)), s)
            n = np.where(ok, n + F32(1), n)
    return (s / n[..., None]).astype(F32)


def check_fill(name, w, h, c, page):
    """the condition of case `name` on the in-between page of upsample(), where the page alone shows it"""
    if name == "zero":
        assert np.array_equal(_bits(page), _bits(smooth_of_mean(c["v"][0], c["v"][1])))
    elif name == "shift":
        assert not _bits(page[h - 1]).any() and not _bits(page[h - 2, :2]).any()
        for x in range(3):                        # one-sided holes: v_neighbour / float(1 / distance), i.e. v * distance
            want = (page[:h - 2, 3] / F32(1.0 / (3 - x))).astype(F32)
            assert np.array_equal(_bits(page[:h - 2, x]), _bits(want))
            assert np.allclose(page[:h - 2, x], page[:h - 2, 3] * (3 - x), rtol=1e-6, atol=0)
    elif name == "converge":
        # at most three rows have weight; the 3x3 mean reaches one row further; every other row stays zero bits
        assert (_bits(page).reshape(h, -1).any(1)).sum() <= 5
    elif name == "leave":
        assert not _bits(page).any()
