"""Seeded inputs of the pyramid-builder tests: the edge cases pinned by the reference's own resampling
library (tests/golden/pyramid_edges_ref.npz and flow_edges_ref.npz hold their outputs only; generators
tests/golden/make_pyramid_golden.py and make_flow_golden.py) and the inputs of the stage tests."""
import numpy as np

# name -> (w, h, levels, seed): thin, tiny and odd lumas down to lines of one sample
LUMA_EDGES = {
    "odd97": (97, 65, 4, 101),       # 97 -> 49 -> 25 -> 13: a line one past three chunks of 32, odd -> odd halvings
    "thin129": (129, 33, 6, 102),    # ... -> 5 x 2: the mirror reflects more than once
    "tiny7": (7, 5, 3, 103),         # 7 x 5 -> 4 x 3 -> 2 x 2
    "tiny3": (3, 2, 2, 104),
    "tiny2": (2, 1, 2, 105),         # -> 1 x 1
    "one": (1, 1, 1, 106),
    "wide257": (257, 3, 3, 107),     # 257 x 3 -> 129 x 2 -> 65 x 1
}

# name -> (w, h, wout, hout, amplitude in px, seed)
FLOW_EDGES = {
    "up": (64, 40, 100, 70, 6.0, 201),           # an enlargement
    "third": (200, 120, 67, 40, 6.0, 202),       # 3 : 1, columns first (40 * 200 < 67 * 120)
    "oddodd": (161, 91, 81, 46, 6.0, 203),       # odd -> odd halving
    "amp40": (120, 68, 60, 34, 40.0, 204),       # close to the +-50 px range, and a tie of the axis order
    "amp80": (120, 68, 60, 34, 80.0, 205),       # beyond it: saturates at 50 px x ratio
    "tie": (80, 40, 40, 20, 3.0, 206),           # hout * w == wout * h: rows first
}


def edge_rgb(name):
    """an RGB8 frame with smooth shading, noise, a hard edge, a black and a saturated region"""
    w, h, _, seed = LUMA_EDGES[name]
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 90 * np.sin(x / 5.0 + seed)[..., None] * np.cos(y[..., None] / 3.0 + np.arange(3))
    rgb = np.clip(base + rng.randn(h, w, 3) * 30, 0, 255)
    rgb[: (h + 1) // 2, : w // 3] = 0
    rgb[h // 2:, w - (w + 2) // 3:] = 255
    return rgb.astype(np.uint8)


def edge_flow(name):
    w, h, _, _, amp, seed = FLOW_EDGES[name]
    return smooth_flow(w, h, amp, seed)


def smooth_flow(w, h, amp, seed, noise=0.3):
    """a smooth flow of the given amplitude (px) with a little noise and one outlier beyond +-50 px"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a, b, c, d = rng.rand(4) * 2 * np.pi
    fx = amp * np.sin(2 * np.pi * x / w + a) * np.cos(2 * np.pi * y / h + b)
    fy = amp * np.cos(2 * np.pi * x / w + c) * np.sin(2 * np.pi * y / h + d)
    flow = np.stack([fx, fy], -1).astype(np.float32) + rng.randn(h, w, 2).astype(np.float32) * np.float32(noise)
    flow[h // 2, w // 3] = (60.0, -70.0)
    return flow


def noise_planes(w, h, seed):
    """(3, h, w) float32 planes for scale() alone: noise over steps, with values below 0 and above 1"""
    rng = np.random.RandomState(seed)
    p = rng.rand(3, h, w).astype(np.float32) * np.float32(1.3) - np.float32(0.15)
    p[:, h // 3:, w // 2:] += np.float32(0.25)
    p[1, : (h + 1) // 2, :] -= np.float32(0.2)
    p[2, :, w // 4: w // 4 + max(1, w // 8)] = np.float32(1.25)
    return p


def harsh_rgb(w, h, seed):
    """an RGB8 frame that hits both branches of both sRGB curves and the clamp of store_gray: dark values on
    either side of the curves' linear segments, black and saturated blocks next to each other (the B-spline
    inverse overshoots below 0 and above 1 there), noise elsewhere"""
    rng = np.random.RandomState(seed)
    rgb = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    rgb[: h // 4] = rng.randint(0, 14, size=(h // 4, w, 3))           # srgbuncurve's linear segment ends at 10.3 / 255
    bh, bw = max(1, h // 8), max(1, w // 8)
    for by in range(h // 2, h, bh):
        for bx in range(0, w // 2, bw):
            rgb[by:by + bh, bx:bx + bw] = 255 * (((by - h // 2) // bh + bx // bw) & 1)
    return rgb
