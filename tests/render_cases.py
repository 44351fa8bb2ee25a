"""What the render tests share (test_gpu_layers, _shutter, _transition, _transition_shutter, _viewport, _viewport_shutter
and the *_ref modules that pin their numpy statements): the fields and frames every family is held to, the layers, the
comparison bit for bit, and the child process that renders under the other form of the chain.  Plain helpers: nothing
here is collected."""
import functools
import os
import subprocess
import sys

import numpy as np

import warp_ref
from videomorphing_amd import morph, synth

f32 = np.float32


@functools.lru_cache(maxsize=None)
def field(w, h, kind, with_path):
    """(v, u or None) of tests/warp_ref.py's kind: computed once, shared, never written"""
    rng = np.random.RandomState(41)
    v = warp_ref.field(kind, w, h, rng)
    u = warp_ref.path(w, h, rng) if with_path else None
    for a in (v, u):
        if a is not None:
            a.setflags(write=False)
    return v, u


@functools.lru_cache(maxsize=None)
def rgb_pair(w, h):
    return synth.make_rgb_pair(w, h)


def frame(ctx, w, h, ex, v, u, schedule=None):
    """a device frame of rgb_pair's extended canvases with the field (v, u) and, if given, the (geometry, colour) schedule"""
    fr = morph.Frame(ctx, w, h, ex)
    rgb0, rgb1 = rgb_pair(w, h)
    fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u)
    if schedule:
        fr.upload_schedule(*schedule)
    return fr


def same_bits(got, want):
    """bit for bit, a NaN for a NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32:
        return got.dtype == want.dtype and np.array_equal(got, want)
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])


def layers(w, h, c, seed):
    """values of both signs over twelve orders of magnitude, +-1e6 among them"""
    rng = np.random.RandomState(seed)
    a = (rng.randn(h, w, c) * 10.0 ** rng.randint(-6, 6, (h, w, c))).astype(f32)
    a[rng.rand(h, w, c) < 0.05] = f32(1e6)
    a[rng.rand(h, w, c) < 0.05] = f32(-1e6)
    return a[..., 0] if c == 1 else a


def hashes_under_render_mode(prog, mode, timeout=300):
    """the HASH lines of `prog`, run in a fresh child process with VM_RENDER set to `mode` ("plain": the plain gather
    kernels) or removed (None: the window form)"""
    env = dict(os.environ)
    env.pop("VM_RENDER", None)
    if mode:
        env["VM_RENDER"] = mode
    r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return [l for l in r.stdout.splitlines() if l.startswith("HASH")]
