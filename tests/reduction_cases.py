"""Shared by tests/test_reduction_mode.py and tests/test_gpu_reduction_mode.py: the digest of an extended frame, the inputs
of the 2304x1464 compositor cases, the script a fresh child process solves one frame with, and a HOST RESTATEMENT of the
ordered reduction's arrival counting and fold order (videomorphing_amd/csrc/vm_mgb_plan.h: VmMgbOrd)."""
import hashlib
import struct

import numpy as np

W, H, EX = 1920, 1080, 192
GROUP = 32          # VM_MGB_ORD_GROUP


def digest(ext1, ext2, iters, rels):
    """SHA-256 of both extended canvases of a frame, plus the iteration counts and the BITS of the returned residuals"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(ext1, np.uint8).tobytes())
    h.update(np.ascontiguousarray(ext2, np.uint8).tobytes())
    return "%s it=%d,%d rel=%s,%s" % (h.hexdigest(), iters[0], iters[1], struct.pack("<f", rels[0]).hex(), struct.pack("<f", rels[1]).hex())


def frame_inputs(f):
    """(extended canvas 1, extended canvas 2, halfway field) of synthetic frame f, as tests/test_gpu_fullsize_compositor.py makes them"""
    import fullsize_fixture as FX
    from videomorphing_amd import morph, synth
    rgb0, rgb1 = synth.make_rgb_pair(W, H, frame=f)
    return morph.make_extended(rgb0, EX), morph.make_extended(rgb1, EX), FX.field(W, H, f)


def solve_digest(ctx, fr, data, tol):
    """upload + both sides of one frame alone (a batch of two systems): its digest"""
    fr.upload(*data, None)
    (i1, r1), (i2, r2), _ = fr.poisson_extend_both(tol=tol)
    return digest(fr.download_ext(1), fr.download_ext(2), (i1, i2), (r1, r2))


CHILD = """
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import reduction_cases as RC
from videomorphing_amd import capi, morph
ctx = morph.Context(0)
ctx.set_reduction(capi.REDUCE_ORDERED)
fr = morph.Frame(ctx, RC.W, RC.H, RC.EX)
print("DIGEST", RC.solve_digest(ctx, fr, RC.frame_inputs(int(sys.argv[1])), float(sys.argv[2])))
fr.close()
ctx.close()
"""


# ---------------------------------------------------------------------------
# The protocol, restated.  A launch holds `grid` workgroups per system (the batch's maximum); the system's own list has n
# entries.  Workgroup i < n publishes its partial and takes a ticket of group i // GROUP; the workgroup whose ticket
# completes the group folds the group's partials in ascending index order and resets the ticket.  Workgroups i >= n do
# nothing.  `arrival` is the order in which the workgroups reach the end of the kernel.

def produce(partials, n, grid, arrival, tickets=None):
    """-> (group sums, ng, folders: which workgroup folded each group, tickets afterwards)"""
    assert grid >= n and sorted(arrival) == list(range(grid))
    ng = (n + GROUP - 1) // GROUP
    tickets = [0] * ng if tickets is None else tickets
    published = {}
    gsum, folders = [None] * ng, [None] * ng
    for i in arrival:
        if i >= n:
            continue
        published[i] = np.float64(partials[i])
        g = i // GROUP
        gsize = min(GROUP, n - g * GROUP)
        old = tickets[g]
        tickets[g] += 1
        if old == gsize - 1:                      # the last arriver: everybody else's partial is published
            tickets[g] = 0
            s = np.float64(0)
            for j in range(g * GROUP, g * GROUP + gsize):
                s = s + published[j]              # a KeyError here would be a read before the write
            gsum[g], folders[g] = s, i
    return gsum, ng, folders, tickets


def consume_device(gsum, ng):
    """the next launch: lane j of 32 adds entries j, j + 32, ... from zero, a butterfly (xor 16 .. 1) joins the lanes"""
    lanes = []
    for j in range(32):
        s = np.float64(0)
        for i in range(j, ng, 32):
            s = s + gsum[i]
        lanes.append(s)
    for o in (16, 8, 4, 2, 1):
        lanes = [lanes[j] + lanes[j ^ o] for j in range(32)]
    assert len({x.tobytes() for x in lanes}) == 1          # every lane ends with the same bits (IEEE addition commutes)
    return lanes[0]


def consume_host(gsum, ng):
    """the stop test: entries 0 .. ng - 1 in ascending order from zero"""
    s = np.float64(0)
    for i in range(ng):
        s = s + gsum[i]
    return s
