"""vm_set_reduction(ctx, VM_REDUCE_ORDERED) on the GPU, at the compositor's stated size (1920x1080, ex = 192: canvases of
2304x1464): the batched multigrid PCG and the quadratic path's mean shift return the SAME BITS from run to run, alone or
in any batch, from process to process and on any context -- and what they return still meets the bounds of
tests/test_gpu_fullsize_compositor.py against the oracle; the default mode is what it was.

A digest (reduction_cases.digest) is the SHA-256 of both extended canvases of a frame, its two iteration counts and the
bits of its two returned residuals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fullsize_fixture as FX
import reduction_cases as RC
from test_gpu_fullsize_compositor import _ring_reference, _ring_stats, _sha_text
from videomorphing_amd import capi, morph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W, H, EX = RC.W, RC.H, RC.EX
TIMED_TOLS = FX.POISSON_TIMED_TOLS
FRAMES = (0, 7)

_inputs = {}


def inputs(f):
    if f not in _inputs:
        _inputs[f] = RC.frame_inputs(f)
    return _inputs[f]


@pytest.fixture(scope="module")
def ord_ctx(vmlib):
    c = morph.Context(0)
    c.set_reduction(capi.REDUCE_ORDERED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def alone(ord_ctx):
    """frames 0 and 7 alone (two systems) in ordered mode at the timed tolerances: digest, canvases, iterations, residuals"""
    out = {}
    fr = morph.Frame(ord_ctx, W, H, EX)
    try:
        for tol in TIMED_TOLS:
            for f in FRAMES:
                fr.upload(*inputs(f), None)
                (i1, r1), (i2, r2), _ = fr.poisson_extend_both(tol=tol)
                e1, e2 = fr.download_ext(1), fr.download_ext(2)
                out[f, tol] = {"digest": RC.digest(e1, e2, (i1, i2), (r1, r2)), "ext": (e1, e2), "iters": (i1, i2), "rels": (r1, r2)}
    finally:
        fr.close()
    return out


def test_run_to_run(ord_ctx, alone):
    fr = morph.Frame(ord_ctx, W, H, EX)
    try:
        for tol in TIMED_TOLS:
            for f in FRAMES:
                again = RC.solve_digest(ord_ctx, fr, inputs(f), tol)
                print(f, tol, again)
                assert again == alone[f, tol]["digest"], (f, tol)
    finally:
        fr.close()


def test_batch_independence(ord_ctx, alone):
    """the same frame alone, in the 4-frame batch (0, 15, 7, 29), in that batch permuted and in an 8-frame batch: frames 15
    and 29 have other type maps, so other block and tile counts -- the launches' grids are THEIR maxima"""
    tol = TIMED_TOLS[0]
    frs = [morph.Frame(ord_ctx, W, H, EX) for _ in range(8)]
    try:
        for order in ((0, 15, 7, 29), (29, 7, 15, 0), (15, 0, 29, 7), (3, 0, 15, 11, 7, 29, 19, 23)):
            use = frs[:len(order)]
            for fr, f in zip(use, order):
                fr.upload(*inputs(f), None)
            res, _ = morph.poisson_extend_frames(use, tol=tol)
            for fr, f, r in zip(use, order, res):
                if f in FRAMES:
                    d = RC.digest(fr.download_ext(1), fr.download_ext(2), (r[0][0], r[1][0]), (r[0][1], r[1][1]))
                    assert d == alone[f, tol]["digest"], (order, f)
    finally:
        for fr in frs:
            fr.close()


def test_process_to_process(alone, tmp_path):
    """two fresh child processes (started, never exec'ed into) solve frame 0 in ordered mode: their digests and this process's"""
    tol = TIMED_TOLS[0]
    script = tmp_path / "ordered_child.py"
    script.write_text(RC.CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = {k: v for k, v in os.environ.items() if k != "VM_REDUCTION"}
    got = []
    for _ in range(2):
        r = subprocess.run([sys.executable, str(script), "0", repr(tol)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        got += [l.split(" ", 1)[1] for l in r.stdout.splitlines() if l.startswith("DIGEST ")]
    assert len(got) == 2 and got[0] == got[1] == alone[0, tol]["digest"], (got, alone[0, tol]["digest"])


def test_parity_holds(alone):
    """ordered mode against the oracle's ring: the bounds of test_poisson_1080p_against_the_oracle_ring at the timed tolerances"""
    checked = 0
    for f in FRAMES:
        z, ref = _ring_reference(f)
        fingerprint_ok = FX.sha(*inputs(f)) == _sha_text(z["inputs"])
        for tol in TIMED_TOLS:
            a = alone[f, tol]
            assert a["rels"][0] <= tol and a["rels"][1] <= tol
            for side in (1, 2):
                out = a["ext"][side - 1]
                assert out[..., 3].max() == 0
                assert np.array_equal(out[EX + 1:EX + H - 1, EX + 1:EX + W - 1, :3], inputs(f)[side - 1][EX + 1:EX + H - 1, EX + 1:EX + W - 1, :3])
                if not fingerprint_ok:           # this host's numpy generates other inputs than the fixture's: no oracle to compare with
                    continue
                worst, f1, f2 = _ring_stats(out, ref[side])
                print({"tol": tol, "frame": f, "side": side, "iters": a["iters"][side - 1], "max_abs_diff": worst, "frac_off_by_1": round(f1, 6)})
                assert worst <= 1, (f, tol, side, worst)
                checked += 1
    print("compared with the oracle's ring: %d canvases" % checked)


def test_quadratic_path_is_reproducible(ord_ctx):
    z = np.load(os.path.join(GOLD, "qpath_1080p_lattice.npz"))
    frame = int(z["frame"])
    v = FX.field(W, H, frame)
    e0, e1, _ = inputs(frame)
    us = []
    other = morph.Context(0)
    try:
        other.set_reduction(capi.REDUCE_ORDERED)
        for ctx, runs in ((ord_ctx, 2), (other, 1)):
            fr = morph.Frame(ctx, W, H, EX)
            try:
                for _ in range(runs):
                    fr.upload(e0, e1, v, None)
                    it, rr, ms = fr.quadratic_path(tol=1e-4, max_it=200)
                    us.append((it, rr, fr.download_qpath()))
            finally:
                fr.close()
    finally:
        other.close()
    for it, rr, u in us[1:]:
        assert (it, rr) == us[0][:2] and np.array_equal(u.view(np.uint32), us[0][2].view(np.uint32))
    it, rr, u = us[0]
    assert rr <= 1e-4
    if FX.sha(v) == _sha_text(z["inputs"]):
        s, lines = int(z["stride"]), [int(k) for k in z["lines"]]
        d = max(float(np.abs(u[::s, ::s] - z["lattice"]).max()), float(np.abs(u[lines] - z["rows"]).max()), float(np.abs(u[:, lines] - z["cols"]).max()))
        print("ordered quadratic path: %d iterations, residual %.2e, max |u - oracle| = %.2e px" % (it, rr, d))
        assert d <= 2e-3, d


def test_default_is_untouched(tmp_path):
    """a context set to ordered and back to atomic meets the existing test's bounds and iterates like a context that never
    called the setter.  Recorded, not asserted: how many bytes differ between two default-mode runs (what the mode removes)."""
    back = morph.Context(0)
    never = morph.Context(0)
    report = []
    try:
        back.set_reduction(capi.REDUCE_ORDERED)
        back.set_reduction(capi.REDUCE_ATOMIC)
        assert back.reduction == never.reduction == capi.REDUCE_ATOMIC
        frb, frn = morph.Frame(back, W, H, EX), morph.Frame(never, W, H, EX)
        try:
            for f in FRAMES:
                z, ref = _ring_reference(f)
                fingerprint_ok = FX.sha(*inputs(f)) == _sha_text(z["inputs"])
                for tol in TIMED_TOLS:
                    runs = []
                    for fr in (frb, frn, frb):
                        fr.upload(*inputs(f), None)
                        (i1, r1), (i2, r2), _ = fr.poisson_extend_both(tol=tol)
                        assert r1 <= tol and r2 <= tol
                        runs.append(((i1, i2), fr.download_ext(1), fr.download_ext(2)))
                    assert runs[0][0] == runs[1][0] == runs[2][0], (f, tol, [r[0] for r in runs])
                    if fingerprint_ok:
                        for side in (1, 2):
                            worst, _, _ = _ring_stats(runs[0][side], ref[side])
                            assert worst <= 1, (f, tol, side, worst)
                    report.append({"frame": f, "tol": tol, "iters": list(runs[0][0]),
                                   "bytes_differing_between_two_default_runs": int((runs[0][1] != runs[2][1]).sum() + (runs[0][2] != runs[2][2]).sum()),
                                   "bytes_differing_between_two_default_contexts": int((runs[0][1] != runs[1][1]).sum() + (runs[0][2] != runs[1][2]).sum())})
        finally:
            frb.close()
            frn.close()
    finally:
        back.close()
        never.close()
    # (printed, and kept as a file where VM_TEST_REPORT_DIR names a directory: profiles/ordered_reduction.json quotes it)
    out_dir = os.environ.get("VM_TEST_REPORT_DIR") or str(tmp_path)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(report, open(os.path.join(out_dir, "reduction_default_run_to_run.json"), "w"), indent=1)
    for r in report:
        print(r)


def test_sharded_job_is_byte_identical(tmp_path):
    """the job of test_bench_config4_on_two_ranks_equals_one_rank with VM_REDUCTION=ordered in the children's environment:
    every one of the 36 frames has the same digest on one rank and on two"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["VM_REDUCTION"] = "ordered"
    docs = {}
    for n in (1, 2):
        dg = str(tmp_path / ("dig%d.json" % n))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--backend", "gloo", "--config", "4", "--pairs", "4",
                            "--size", "480x270", "--steps", "1", "--warmup", "0", "--digest", dg],
                           capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        merged = {"fields": {}, "frames": {}}
        for f in ([dg] if n == 1 else [dg + ".0", dg + ".1"]):
            doc = json.load(open(f))
            for k in merged:
                merged[k].update(doc[k])
        docs[n] = merged
    assert docs[1]["fields"] == docs[2]["fields"] and sorted(docs[1]["fields"]) == ["0", "1", "2", "3"]
    assert sorted(docs[1]["frames"]) == sorted(docs[2]["frames"]) and len(docs[1]["frames"]) == 36
    differ = [k for k in docs[1]["frames"] if docs[1]["frames"][k] != docs[2]["frames"][k]]
    assert not differ, differ
