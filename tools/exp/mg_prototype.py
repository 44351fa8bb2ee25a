"""The numpy model of the device's multigrid-preconditioned CG (tests/mgb_ref.py, which the tests compare vm_mgb.hip with) on
the Poisson extension's system of one side of a fixture frame: iteration counts of smoother / cycle variants BEFORE any kernel is written (build container, CPU only).

The hierarchy is the device's: 2x2 aggregation, piecewise-constant transfer, Galerkin operator with the edge weights
halved, down to a grid of <= 64 cells that gets 2 symmetric sweeps each way; the smoother is red-black Gauss-Seidel,
`nu` full sweeps before (red, black) and after (black, red) the coarse correction, per level.  PCG in float64 on
channel 0, 1 and 2 (the worst channel counts, as on the device).

usage: python tools/exp/mg_prototype.py [--size 1920x1080] [--ex 192] [--frame 0] [--side 1] [--nu 1,1,1,...;2,2,2,...]
  --nu  one comma list per variant, separated by ';': sweeps per level from level 0 down, the last entry repeats
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
import fullsize_fixture as FX  # noqa: E402
from videomorphing_amd import synth  # noqa: E402
import mgb_ref  # noqa: E402  (the model itself: the tests compare the device with it)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def make_extended(rgb, ex):
    h, w = rgb.shape[:2]
    out = np.full((h + 2 * ex, w + 2 * ex, 4), 255, np.uint8)
    out[ex:ex + h, ex:ex + w, :3] = rgb
    out[ex:ex + h, ex:ex + w, 3] = 0
    return out


def system(w, h, ex, frame, side):
    """type map, diagonal and right-hand side of oracle/vm_oracle_poisson.c (PoissonExt.cpp:146-312), vectorised"""
    rgb0, rgb1 = synth.make_rgb_pair(w, h, frame=frame)
    v = FX.field(w, h, frame)
    e = [make_extended(rgb0, ex), make_extended(rgb1, ex)]
    other = e[2 - side][ex:ex + h, ex:ex + w].copy()
    ext, typ, _ = oracle.poisson_prepare(e[side - 1], w, h, ex, other, v, side)
    col = ext[..., :3].astype(np.float64)
    marker = (ext[..., 0] == 255) & (ext[..., 1] == 0) & (ext[..., 2] == 255) & (ext[..., 3] == 0)
    t2 = (typ > 1) & ~marker
    gx = np.zeros(col.shape)
    gy = np.zeros(col.shape)
    ok = t2[:, 1:] & t2[:, :-1]
    gx[:, 1:][ok] = (col[:, 1:] - col[:, :-1])[ok]
    ok = t2[1:] & t2[:-1]
    gy[1:][ok] = (col[1:] - col[:-1])[ok]
    unk = typ > 0
    E = unk[:, :-1] & unk[:, 1:]            # edge (x, y) - (x + 1, y)
    S = unk[:-1] & unk[1:]
    B = np.zeros(col.shape)
    B[typ == 1] += col[typ == 1]
    B[1:][S] += gy[1:][S]                   # north neighbour present
    B[:, 1:][E] += gx[:, 1:][E]             # west
    B[:, :-1][E] -= gx[:, 1:][E]            # east
    B[:-1][S] -= gy[1:][S]                  # south
    B[~unk] = 0
    tie = (typ == 1).astype(np.float64)
    return unk, E.astype(np.float64), S.astype(np.float64), tie, B


def pcg(levels, B, nu, tols, max_it=60):
    """iterations to each tolerance, from zero (the statement of the iteration: tests/mgb_ref.py)"""
    nul = [nu[min(l, len(nu) - 1)] for l in range(len(levels))]
    hist = mgb_ref.pcg(levels, B, np.zeros_like(B), nul, min(tols), max_it)[1]
    return [next((it for it, rel in enumerate(hist) if rel <= t), -1) for t in tols]


def main():
    w, h = (int(t) for t in arg("--size", "1920x1080").split("x"))
    ex = int(arg("--ex", "192"))
    frame, side = int(arg("--frame", "0")), int(arg("--side", "1"))
    variants = [[int(t) for t in v.split(",")] for v in arg("--nu", "1;2").split(";")]
    t0 = time.time()
    unk, E, S, tie, B = system(w, h, ex, frame, side)
    levels = mgb_ref.hierarchy(mgb_ref.Level(E, S, tie))
    print("canvas %dx%d, %d unknowns, %d levels (coarsest %dx%d), set-up %.0f s" % (
        w + 2 * ex, h + 2 * ex, int(unk.sum()), len(levels), levels[-1].w, levels[-1].h, time.time() - t0), flush=True)
    tols = (1e-4, 1e-5, 1e-6)
    for nu in variants:
        t0 = time.time()
        its = pcg(levels, B, nu, tols)
        print("nu per level %-24s PCG iterations to 1e-4 / 1e-5 / 1e-6: %s   (%.0f s)" % (",".join(map(str, nu)), " / ".join(map(str, its)), time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
