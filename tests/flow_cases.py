"""The seeded hard-input cases of the optical-flow stage tests, shared by the CPU checks
(tests/test_flow_spec.py: every case keeps its flip-excused share within the cap on the float64 spec
alone) and the GPU checks (tests/test_gpu_flow_stages.py).  Not a test module.

A case is (id, kind, seed, w, h, keywords of flow_ref.params).  pyr_scale and poly_sigma are given as
written; spec_params() rounds them to float32, which is what crosses the C ABI."""
import numpy as np

import flow_ref as R

EXCUSED_CAP = 0.01  # at most this share of a case's pixels may be excused; 0 for the num_iters = 1 cases


def frames(kind, seed, w, h):
    """a frame pair (float32 luma, values exactly representable) of one of the hard kinds"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":        # white noise, moved by (2, 1) px
        a = rng.random((h, w)) * 255.0
        b = np.roll(a, (1, 2), (0, 1))
    elif kind == "edge":       # low noise and a slanted step edge, moved by (3, -2) px
        a = rng.random((h, w)) * 64.0 + 150.0 * (x + 0.5 * y > 0.6 * w)
        b = np.roll(a, (-2, 3), (0, 1))
    elif kind == "large":      # a smooth texture moved by (12, -5) px: a wide band of x + d is outside
        a = R.blur(rng.random((h, w)), R.gauss_taps(2.0, 6))
        a = 16.0 + 224.0 * (a - a.min()) / (a.max() - a.min())
        b = np.roll(a, (-5, 12), (0, 1))
    elif kind == "blocks":     # sharp 8-px blocks over the whole 0..255 range, moved by (2, -1) px
        v = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8)).astype(np.float64)
        v[::3, ::2], v[1::3, 1::2] = 0.0, 255.0
        a = np.kron(v, np.ones((8, 8)))[:h, :w]
        b = np.roll(a, (-1, 2), (0, 1))
    elif kind == "zoom":       # a textured step edge shrinking by 6 % about the centre: up to 6 px, inward at every border
        a = R.blur(rng.random((h, w)), R.gauss_taps(1.5, 4))
        a = 16.0 + 160.0 * (a - a.min()) / (a.max() - a.min()) + 60.0 * (x + 0.5 * y > 0.6 * w)
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        sx, sy = np.clip(cx + (x - cx) / 0.94, 0, w - 1), np.clip(cy + (y - cy) / 0.94, 0, h - 1)
        x0, y0 = np.minimum(np.floor(sx).astype(int), w - 2), np.minimum(np.floor(sy).astype(int), h - 2)
        fx, fy = sx - x0, sy - y0
        b = ((1 - fy) * ((1 - fx) * a[y0, x0] + fx * a[y0, x0 + 1]) +
             fy * ((1 - fx) * a[y0 + 1, x0] + fx * a[y0 + 1, x0 + 1]))
    elif kind == "const":      # A = 0 everywhere
        a = b = np.full((h, w), 77.0)
    elif kind == "same":       # identical frames: every db is exactly 0
        a = b = rng.random((h, w)) * 255.0
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def rgb_frames(kind, seed, w, h):
    """an RGB8 frame pair: 'rgb' independent random R, G, B (low-pass, so that neighbours correlate),
    moved by (2, 1) px; 'red' / 'blue' one texture in the R or the B channel alone, the others 0"""
    rng = np.random.default_rng(seed)
    def tex():
        t = R.blur(rng.random((h, w)), R.gauss_taps(1.0, 3))
        return np.clip(np.rint(255.0 * (t - t.min()) / (t.max() - t.min())), 0, 255).astype(np.uint8)
    if kind == "rgb":
        a = np.stack([tex(), tex(), tex()], -1)
    else:
        a = np.zeros((h, w, 3), np.uint8)
        a[..., 0 if kind == "red" else 2] = tex()
    return np.ascontiguousarray(a), np.ascontiguousarray(np.roll(a, (1, 2), (0, 1)))


def spec_params(kw):
    p = R.params(**kw)
    p["pyr_scale"], p["poly_sigma"] = R.f32(p["pyr_scale"]), R.f32(p["poly_sigma"])
    return p


def _c(id, kind, seed, w, h, **kw):
    return (id, kind, seed, w, h, kw)


# 1. stage isolation: one scale, 1..3 iterations; one coarse iteration behind the blur and the resizes
STAGE = [
    _c("poly-iter0-noise", "noise", 11, 96, 64, num_levels=0, num_iters=1),
    _c("poly-iter0-edge", "edge", 12, 100, 70, num_levels=0, num_iters=1),
    _c("poly-iter0-blocks", "blocks", 13, 96, 129, num_levels=0, num_iters=1),
    _c("poly-iter0-large-n7", "large", 14, 96, 64, num_levels=0, num_iters=1, poly_n=7, poly_sigma=1.5),
    _c("const", "const", 0, 65, 33, num_levels=1, num_iters=2),
    _c("same", "same", 15, 100, 70, num_levels=1, num_iters=3),
    _c("gather2-noise", "noise", 121, 96, 64, num_levels=0, num_iters=2),
    _c("gather3-noise", "noise", 22, 96, 64, num_levels=0, num_iters=3),
    _c("gather2-large", "large", 23, 96, 64, num_levels=0, num_iters=2),
    _c("gather3-large", "large", 24, 96, 64, num_levels=0, num_iters=3),
    _c("gather2-blocks", "blocks", 25, 100, 70, num_levels=0, num_iters=2),
    _c("gather3-edge", "edge", 126, 100, 70, num_levels=0, num_iters=3),
    _c("level1-s0.5-noise", "noise", 31, 100, 70, num_levels=1, num_iters=1, pyr_scale=0.5),
    _c("level1-s0.8-noise", "noise", 32, 96, 64, num_levels=1, num_iters=1, pyr_scale=0.8),
    _c("level1-s0.7-edge", "edge", 33, 65, 70, num_levels=1, num_iters=1, pyr_scale=0.7),     # 65 * 0.7 = 45.5
    _c("level1-s0.3-large", "large", 34, 115, 120, num_levels=1, num_iters=1, pyr_scale=0.3),  # 115 * 0.3 = 34.5
    _c("level1-s0.8-at32", "blocks", 35, 40, 44, num_levels=1, num_iters=1, pyr_scale=0.8),   # 40 * f32(0.8) just above 32
    _c("level3-s0.8-noise", "noise", 36, 83, 70, num_levels=3, num_iters=1, pyr_scale=0.8),   # 83 * 0.8^3 = 42.496
]

# 2. window sizes x poly_n x tile-edge frame sizes, two iterations behind one coarse level
GRID = [
    _c("win3-n5-32x32", "noise", 41, 32, 32, num_levels=1, num_iters=2, win_size=3),
    _c("win3-n7-33x47", "noise", 42, 33, 47, num_levels=0, num_iters=2, win_size=3, poly_n=7, poly_sigma=1.5),
    _c("win13-n7-65x33", "noise", 43, 65, 33, num_levels=0, num_iters=2, win_size=13, poly_n=7, poly_sigma=1.5),
    _c("win13-n5-32x32", "edge", 44, 32, 32, num_levels=0, num_iters=2),
    _c("win17-n5-257x64", "edge", 345, 257, 64, num_levels=1, num_iters=2, win_size=17),
    _c("win17-n7-96x129", "edge", 146, 96, 129, num_levels=1, num_iters=2, win_size=17, poly_n=7, poly_sigma=1.5),
    _c("win19-n5-100x70", "blocks", 2247, 100, 70, num_levels=1, num_iters=2, win_size=19),
    _c("win19-n7-40x300", "noise", 1948, 40, 300, num_levels=1, num_iters=2, win_size=19, poly_n=7, poly_sigma=1.5),
    _c("win31-n5-300x40", "noise", 49, 300, 40, num_levels=1, num_iters=2, win_size=31),
    _c("win31-n7-65x33", "edge", 50, 65, 33, num_levels=0, num_iters=2, win_size=31, poly_n=7, poly_sigma=1.5),
    _c("win31-n5-32x32", "noise", 51, 32, 32, num_levels=0, num_iters=1, win_size=31),
    _c("win17-n5-33x47", "large", 52, 33, 47, num_levels=0, num_iters=3, win_size=17),
    _c("win19-n5-257x64", "edge", 153, 257, 64, num_levels=2, num_iters=1, win_size=19, pyr_scale=0.7),
]

# 3. whole chains: default iterations on one scale, a table that stops itself, the full defaults
FULL = [
    _c("levels0-default-iters", "zoom", 61, 96, 64, num_levels=0),
    _c("levels9-100x70", "zoom", 62, 100, 70, num_levels=9),
    _c("defaults-zoom-192x120", "zoom", 63, 192, 120),
    _c("defaults-zoom-127x99", "zoom", 64, 127, 99),
]

# 4. the one large-radius blur: pyr_scale 0.03 at 1072 x 1072 is a 32 x 32 level behind a radius-40 blur (81 taps,
# 36.3 KB of dynamic LDS in k_blur_cols).  Radius 61 (pyr_scale 0.02) needs 1664 x 1664, whose numpy reference costs
# more than three times the rest of the GPU module together; this is the next radius down that keeps the module cheap.
BIG = [_c("blur-r40-1072", "zoom", 76, 1072, 1072, num_levels=1, num_iters=1, pyr_scale=0.03)]

CASES = STAGE + GRID + FULL
IDS = [c[0] for c in CASES]


def reference(case):
    """(a, b, float64 flow, excused mask, float32 flow) of a case"""
    _, kind, seed, w, h, kw = case
    a, b = frames(kind, seed, w, h)
    p = spec_params(kw)
    d64, mask = R.flow(a, b, p, excuse=True)
    return a, b, d64, mask, R.flow(a, b, p, np.float32)


def excused_cap(case):
    return 0.0 if case[5].get("num_iters", R.DEFAULTS["num_iters"]) == 1 else EXCUSED_CAP
