"""The multigrid preconditioner of the compositor's linear solver (vm_mgb.hip, driven by vm_poisson_api.cpp), stage by stage
against the float64 statement of it in tests/mgb_ref.py, through the read-only hooks vm_dbg_mgb_setup / _level / _cycle:
the hierarchy level by level, one cycle's right-hand sides and results level by level, the symmetry of M, the cycle
variants, the reduction modes and the iteration counts.  A preconditioned CG reaches its answer with almost any
preconditioner: the end-to-end tests cannot see a wrong coarse weight, a post-smoothing in the wrong colour order, a
two-sweep kernel that disagrees with two sweeps, a tail that drops a level or an apron that is a cell short.  These can.

Tolerances (mgb_ref.tolerance): per quantity and level, 8 x the deviation of the statement's own float32 run from its
float64 run, relative to the quantity's max norm, at least 16 float32 ulps.  Nothing is sized from the device's output."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mgb_ref
import mgb_stages as M
from videomorphing_amd import capi, morph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a: canvases (w, h, ex) at the tile and block edges, all tail, three tile levels, the pairs limit, every level odd
EDGE_SHAPES = [(cw, ch, 3) for cw in (63, 64, 65, 127, 129) for ch in (15, 16, 17, 33)]
HIERARCHY_SHAPES = [(26, 18, 4), (380, 260, 40), (3, 1700, 1), (129, 65, 5)]


def _hierarchies(ctx, shapes):
    report = []
    for k, (cw, ch, ex) in enumerate(shapes):
        fr, e0, e1, _ = M.open_case(ctx, cw, ch, ex, 7 + k)
        try:
            for side, e in ((1, e0), (2, e1)):
                S = M.statement_of_canvas(e, mgb_ref.NU_POISSON)
                info = M.check_hierarchy("%dx%d side %d" % (cw, ch, side), fr, side, S, report)
                if (cw, ch) == (26, 18):
                    assert info["tail"] == 0                      # the k_mgb_dot_rz path
                if (cw, ch) == (380, 260):
                    assert info["tail"] == 3 and info["nu"][:3] == [1, 1, 2]
                if (cw, ch) == (3, 1700):
                    assert info["tail"] == 1                      # VM_MGB_TAIL_PAIRS keeps level 0 out of the tail
                if (cw, ch) == (129, 65):
                    assert all(w % 2 and h % 2 for w, h in info["sizes"])
        finally:
            fr.close()


def test_hierarchy_at_tile_and_block_edges(gpu_ctx):
    """a. dg, we, ws of every level, nlev, tail, nu, block and tile counts: 63 .. 129 wide by 15 .. 33 high"""
    _hierarchies(gpu_ctx, EDGE_SHAPES)


def test_hierarchy_tail_rules_and_odd_levels(gpu_ctx):
    """a. ... all tail (26 x 18), three tile levels with level 2 on two sweeps (380 x 260), the pairs limit (3 x 1700), every
    level odd x odd (129 x 65)"""
    _hierarchies(gpu_ctx, HIERARCHY_SHAPES)


def test_hierarchy_of_the_quadratic_path(gpu_ctx):
    fr, _, _, _ = M.open_case(gpu_ctx, 162, 112, 1, 40)
    try:
        M.check_hierarchy("160x110 qpath", fr, M.QPATH, M.statement_of_grid(160, 110, mgb_ref.NU_QPATH), [])
    finally:
        fr.close()


def test_one_cycle_stage_by_stage(gpu_ctx):
    """b. b[l + 1] above the tail, x[l] down to the tail, z, q = A z: 380 x 260, partial last tiles both ways (65 x 17, 129 x
    33), all tail (26 x 18), 3 x 1700; the quadratic path's system at 160 x 110"""
    M.run_cycle_shapes(gpu_ctx, [])


def test_preconditioner_is_symmetric_and_positive(gpu_ctx):
    """c. <u, M v> == <M u, v> and <u, M u> > 0 for four seeded pairs and for u on one tile's corner cells, 380 x 260 and
    65 x 17: the red / black order mistake that PCG hides"""
    M.run_symmetry_shapes(gpu_ctx, [])


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); import mgb_stages; mgb_stages.child_main()"


@pytest.mark.parametrize("nu", ["2", "2,1,3"])
def test_cycle_variants_stage_by_stage(nu):
    """d. b and c again under VM_MGB_NU = 2 (level 0 through k_mgb_restrict2<true> / k_mgb_prolong2<true>, which the default
    never runs on Poisson systems) and 2,1,3 (a tail with three sweeps): a fresh process per setting (the library reads the
    variable once) runs all shapes"""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, VM_MGB_NU=nu), capture_output=True, text=True,
                       timeout=600, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and "MGB_STAGES_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-2500:])


def test_cycle_fields_do_not_depend_on_the_reduction_mode(gpu_ctx):
    """e. z and q of a cycle are bit-identical between VM_REDUCE_ATOMIC and VM_REDUCE_ORDERED: the field outputs do not
    depend on how the dot products are added up"""
    was = gpu_ctx.reduction
    fr, e0, _, _ = M.open_case(gpu_ctx, 380, 260, 40, 61)
    try:
        S = M.statement_of_canvas(e0, mgb_ref.NU_POISSON)
        r = M.residual(S.unk, 400)
        gpu_ctx.set_reduction(capi.REDUCE_ATOMIC)
        za, qa = M.dev_cycle(fr, 1, r)
        gpu_ctx.set_reduction(capi.REDUCE_ORDERED)
        zo, qo = M.dev_cycle(fr, 1, r)
        assert np.abs(za).max() > 0 and np.array_equal(za, zo) and np.array_equal(qa, qo)
    finally:
        gpu_ctx.set_reduction(was)
        fr.close()


def _solve_two_frames(ctx):
    frames = [M.open_case(ctx, 380, 260, 40, 71 + k)[0] for k in range(2)]
    try:
        per_frame, _ = morph.poisson_extend_frames(frames, tol=1e-5)
        its = [int(s[0]) for f in per_frame for s in f]
        ext = np.stack([fr.download_ext(side) for fr in frames for side in (1, 2)])
    finally:
        for fr in frames:
            fr.close()
    return its, ext


_UNFUSED_CHILD = """
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import test_gpu_mgb_stages as T
from videomorphing_amd import morph
its, ext = T._solve_two_frames(morph.Context(0))
np.savez(sys.argv[2], its=np.array(its), ext=ext)
print("UNFUSED_OK")
"""


def test_fused_and_separate_update_agree(gpu_ctx, tmp_path):
    """e. a full solve of a 2-frame batch at 380 x 260 with the PCG update as a kernel of its own (VM_MGB_FUSE_MIN_SYS = 0, a
    fresh process) takes the same iteration counts as the fused default and gives colours within one level"""
    its, ext = _solve_two_frames(gpu_ctx)
    out = str(tmp_path / "unfused.npz")
    r = subprocess.run([sys.executable, "-c", _UNFUSED_CHILD, ROOT, out], env=dict(os.environ, VM_MGB_FUSE_MIN_SYS="0"),
                       capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and "UNFUSED_OK" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    got = np.load(out)
    assert all(0 < i < 40 for i in its) and list(got["its"]) == its, (its, list(got["its"]))
    assert np.abs(got["ext"].astype(int) - ext.astype(int)).max() <= 1


@pytest.mark.parametrize("case", M.ITERATION_TABLE, ids=lambda c: "%s-%dx%d-%g" % (c[0], c[1], c[2], c[6]))
def test_iteration_counts_equal_the_statements(gpu_ctx, case):
    """f. the device's PCG stops within one iteration of the float64 statement's N.  The inputs were chosen on the CPU so that
    N is not near a crossing (mgb_stages.safe_count; test_mgb_ref.py re-derives the table)"""
    kind, cw, ch, ex, seed, side, tol, N = case
    if kind == "poisson":
        fr = M.open_case(gpu_ctx, cw, ch, ex, seed)[0]
        try:
            it, rel, _ = fr.poisson_extend(side, tol=tol)
        finally:
            fr.close()
    else:
        fr = morph.Frame(gpu_ctx, cw, ch, 0)
        try:
            fr.upload(None, None, M.qpath_field(cw, ch, seed, ex), None)
            it, rel, _ = fr.quadratic_path(tol=tol)
        finally:
            fr.close()
    print("device %d iterations (rel %.3g), statement %d" % (it, rel, N))
    assert rel <= tol and abs(it - N) <= 1, (it, N, rel)
