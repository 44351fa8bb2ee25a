"""Host-side mirror of the reference's L3 solver API over the C-ABI.

Same names, argument meaning and progress/cancellation behaviour as
Algorithm/parameters.h (Parameters, KernParameters, Conp, Connect,
BoundaryCondition), Algorithm/Pyramid.h (Pyramid, PyramidLevel),
Algorithm/morph.h (Morph) and Algorithm/MatchingThread.h (CMatchingThread), so
that tests read like drivers of the reference.  This module holds no
numerics: everything runs in libvmorph_hip.so.  (The C++ facade with the same
shape is include/vmorph/*.hpp.)

Scope: one frame pair per Pyramid (depth 1, the independent-pair formulation).
"""
import ctypes as C
import os
import threading
import time
import weakref

import numpy as np

from . import capi
from .capi import BCOND_NONE, BCOND_CORNER, BCOND_BORDER, MATH_EXACT, MATH_FAST, REDUCE_ATOMIC, REDUCE_ORDERED  # noqa: F401
from .capi import ERR_SSIM, ERR_TPS, ERR_UI, ERR_TEMP, ERR_ALL  # noqa: F401
from . import synth


class Conp(object):
    """struct Conp, parameters.h:22-26: p = (x, y, frame, is_key), weight."""

    def __init__(self, x, y, z=0, w=1, weight=1.0):
        self.p = (int(x), int(y), int(z), int(w))
        self.weight = float(weight)


class Connect(object):
    """struct Connect, parameters.h:16-20: li/ri = (track, frame) indices."""

    def __init__(self, li, ri):
        self.li = tuple(li)
        self.ri = tuple(ri)


class Parameters(object):
    """struct Parameters, parameters.h:29-52, defaults of UI/MdiEditor.cpp:131-140."""

    def __init__(self):
        self.w_ui, self.w_tps, self.w_ssim, self.w_temp = 1e5, 0.05, 100.0, 10.0
        self.ssim_clamp = 0.0
        self.eps = 0.01
        self.max_iter = 1000
        self.start_res = 8
        self.max_iter_drop_factor = 2.0
        self.bcond = BCOND_NONE
        self.lp, self.rp, self.cnt = [], [], []
        self.verbose = False

    def add_point_pair(self, lx, ly, rx, ry, weight=1.0, frame=0):
        """Convenience: one key-point track per side plus its connection."""
        self.lp.append([Conp(lx, ly, frame, 1, weight)])
        self.rp.append([Conp(rx, ry, frame, 1, weight)])
        k = len(self.lp) - 1
        self.cnt.append([Connect((k, 0), (k, 0))])

    def constraints(self, conz=0):
        """Resolve lp/rp/cnt as morph.cu:354-366 does for page `conz`."""
        out = []
        for row in self.cnt:
            for c in row:
                l = self.lp[c.li[0]][c.li[1]]
                r = self.rp[c.ri[0]][c.ri[1]]
                if l.p[2] != conz:
                    continue
                out.append((l.p[0], l.p[1], r.p[0], r.p[1], min(l.weight, r.weight)))
        return np.asarray(out, dtype=np.float32).reshape(-1, 5)


class KernParameters(capi.KernParams):
    """struct KernParameters(const Parameters&), parameters.h:54-72."""

    def __init__(self, p=None):
        capi.KernParams.__init__(self)
        if p is not None:
            self.w_temp, self.w_ui, self.w_tps, self.w_ssim = p.w_temp, p.w_ui, p.w_tps, p.w_ssim
            self.ssim_clamp, self.eps, self.bcond = p.ssim_clamp, p.eps, int(p.bcond)


class Context(object):
    """One HIP device + stream (vm_ctx)."""

    def __init__(self, device=0, math_mode=MATH_EXACT):
        self._L = capi.load()
        h = C.c_void_p()
        capi.check(self._L.vm_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        # (what vm_ctx_create read from the environment; any other value made it fail)
        self.reduction = REDUCE_ORDERED if os.environ.get("VM_REDUCTION") == "ordered" else REDUCE_ATOMIC
        self.set_math_mode(math_mode)

    def close(self):
        if getattr(self, "_h", None):
            self._L.vm_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def set_params(self, kp):
        capi.check(self._L.vm_set_params(self._h, C.byref(kp)))

    def set_math_mode(self, mode):
        capi.check(self._L.vm_set_math_mode(self._h, int(mode)))
        self.math_mode = int(mode)

    def set_tuning(self, sweep_mode=0, threads=0, parts=0):
        capi.check(self._L.vm_set_tuning(self._h, int(sweep_mode), int(threads), int(parts)))

    def runs_beside(self, other):
        """vm_dbg_streams_overlap: do this context's stream and `other`'s run their kernels side by side (True) or
        did the runtime put them on one hardware queue (False)?"""
        ov = C.c_int(0)
        capi.check(self._L.vm_dbg_streams_overlap(self._h, other._h, C.byref(ov)))
        return bool(ov.value)

    def poisson_profile(self, on):
        """vm_dbg_poisson_profile: arm (on = True) the HIP-event probe around the linear solver's dominant kernel (the launch
        that carries the PCG update), or disarm it and return (summed us, launches, active systems summed over the launches,
        launches of the form with the update fused into the level-0 restriction)"""
        us, n, act, fused = C.c_double(0), C.c_int(0), C.c_double(0), C.c_int(0)
        capi.check(self._L.vm_dbg_poisson_profile(self._h, int(bool(on)), C.byref(us), C.byref(n), C.byref(act), C.byref(fused)))
        return us.value, n.value, act.value, fused.value

    def set_commit_order(self, order=0):
        """diagnostic (EXACT): the order a phase's commits are folded in -- 0 row-major (the oracle's),
        1 reversed, 2 column-major, 3 column-major reversed (vm_set_commit_order)"""
        capi.check(self._L.vm_set_commit_order(self._h, int(order)))

    def set_reduction(self, mode=REDUCE_ORDERED):
        """how the compositor's linear solver adds up its dot products (vm_set_reduction): REDUCE_ATOMIC (0, the default:
        arrival order, run-dependent in the last bit) or REDUCE_ORDERED (1: one fixed order per system -- the same bytes from
        run to run, alone or in any batch, on any context)"""
        capi.check(self._L.vm_set_reduction(self._h, int(mode)))
        self.reduction = int(mode)

    def set_sparse_resident(self, mode=0):
        """test hook of the SPARSE schedule's resident visits (FAST): 0 automatic, 1 never, 2 re-centre the LDS copy
        after every commit, 3 give residency up at the first commit (vm_dbg_sparse_resident)"""
        capi.check(self._L.vm_dbg_sparse_resident(self._h, int(mode)))

    def set_sweep_variant(self, mode=0):
        """test hook of the FAST sweep variants: 0 by the level (the kernels compiled without the temporal term where
        no page carries it), 1 always the general kernels (vm_dbg_sweep_variant)"""
        capi.check(self._L.vm_dbg_sweep_variant(self._h, int(mode)))

    def sparse_resident_visits(self):
        """tile visits of this context's solves served from the resident LDS copy so far (vm_dbg_sparse_resident_visits)"""
        return int(self._L.vm_dbg_sparse_resident_visits(self._h))

    def sync(self):
        capi.check(self._L.vm_ctx_sync(self._h))

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(0), C.c_uint64(0)
        capi.check(self._L.vm_device_info(self._h, name, C.byref(cus), C.byref(mem)))
        return name.value.decode(), cus.value, mem.value


def _cons_array(cons):
    cons = np.asarray(cons if cons is not None else [], dtype=np.float32).reshape(-1, 5)
    n = len(cons)
    arr = (capi.Constraint * max(n, 1))()
    for k in range(n):
        arr[k] = capi.Constraint(*[float(x) for x in cons[k]])
    return arr, n


class _ErrorView(object):
    """The error view of a level or a video page (the reference only has the menu entry,
    UI/MdiEditor.cpp:1928-1933): _err(name) returns the C-ABI entry vm_{level,video}_<name> and the arguments that
    address this level / page.  VmError(VM_E_STATE) while the level holds no initialised state."""

    def energy(self):
        """the five totals {"ssim", "tps", "ui", "temp", "all"} (float64, the same bits from run to run)"""
        fn, at = self._err("energy")
        out = (C.c_double * 5)()
        capi.check(fn(*at, out))
        return dict(zip(capi.ERR_NAMES, [float(x) for x in out]))

    def error_map(self, what=ERR_SSIM):
        """plane `what` (ERR_*) of the per-pixel energy terms, (h, w) float32"""
        fn, at = self._err("error_map")
        out = np.zeros((self.height, self.width), dtype=np.float32)
        capi.check(fn(*at, int(what), out.ctypes.data, 0))
        return out

    def error_image(self, w0, h0, what=ERR_SSIM, gain=1.0):
        """the heat-ramp image of plane `what` times `gain`, resized to w0 x h0: (h0, w0, 3) uint8"""
        fn, at = self._err("error_image")
        out = np.zeros((int(h0), int(w0), 3), dtype=np.uint8)
        capi.check(fn(*at, int(what), float(gain), int(w0), int(h0), out.ctypes.data, 0))
        return out


class PyramidLevel(_ErrorView):
    """struct PyramidLevel, Pyramid.h:52-98 (geometry + device-state access)."""

    def __init__(self, pyr, el, w, h):
        # a weak back-reference: no Pyramid <-> PyramidLevel cycle, so a pyramid is released by
        # reference counting the moment its last user lets go -- before its Context, which it
        # keeps alive -- and never by the cycle collector in an arbitrary order
        self._pyr_ref, self._el = weakref.ref(pyr), el
        self.width, self.height, self.depth = int(w), int(h), 1
        self.rowstride = (self.width + 31) // 32 * 32         # pyramid.cu:535
        self.pagestride = self.rowstride * self.height
        self.inv_wh = np.float32(1.0) / np.float32(self.width * self.height)
        self.impmask_rowstride = (self.width + 4) // 5 + 2
        self.impmask_pagestride = self.impmask_rowstride * ((self.height + 4) // 5 + 2)
        self.factor_d = 1.0

    @property
    def _pyr(self):
        # lifetime rule: a level is a view into its Pyramid and does not keep
        # it alive -- hold the Pyramid for as long as its levels are used
        p = self._pyr_ref()
        if p is None:
            raise capi.VmError(capi.VM_E_STATE, "this PyramidLevel outlived its Pyramid: keep a reference to the "
                                                "Pyramid while its levels are in use")
        return p

    def _lvl(self):
        if self._el < 1:
            raise capi.VmError(capi.VM_E_STATE, "pyramid[0] is the full-resolution placeholder")
        return self._el - 1

    def field(self, name):
        """Copy a device-state array to the host: (h,w), (h,w,2) or the mask words."""
        fid, ch = capi.FIELDS[name]
        L = self._pyr._L
        if name == "impmask":
            out = np.zeros(((self.height + 4) // 5 + 2, self.impmask_rowstride), dtype=np.uint32)
        elif ch == 2:
            out = np.zeros((self.height, self.width, 2), dtype=np.float32)
        else:
            out = np.zeros((self.height, self.width), dtype=np.float32)
        capi.check(L.vm_level_get_field(self._pyr._h, self._lvl(), fid, out.ctypes.data))
        return out

    def _err(self, name):
        return getattr(self._pyr._L, "vm_level_" + name), (self._pyr._h, self._lvl())

    def set_impmask(self, words):
        """test hook: overwrite the improving mask (the array field("impmask") returns), vm_dbg_level_set_mask"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        assert words.shape == ((self.height + 4) // 5 + 2, self.impmask_rowstride)
        capi.check(self._pyr._L.vm_dbg_level_set_mask(self._pyr._h, self._lvl(), words.ctypes.data))

    @property
    def v(self):
        out = np.zeros((self.height, self.width, 2), dtype=np.float32)
        capi.check(self._pyr._L.vm_level_get_v(self._pyr._h, self._lvl(), out.ctypes.data, 0))
        return out

    @v.setter
    def v(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        assert arr.shape == (self.height, self.width, 2)
        capi.check(self._pyr._L.vm_level_set_v(self._pyr._h, self._lvl(), arr.ctypes.data, 0))


class Pyramid(object):
    """class Pyramid, Pyramid.h:14-48.  pyramid[0] is the full-resolution
    placeholder (pyramid.cu:220); pyramid[1..size()-1] run finest to coarsest;
    the last level holds no images (pyramid.cu:329)."""

    def __init__(self, ctx):
        self._ctx = ctx
        self._L = capi.load()
        self._h = None
        self._levels = []
        self._vector, self._qpath = [], []
        self._extends1, self._extends2, self._results = [], [], []

    def size(self):
        return len(self._levels)

    __len__ = size

    def __getitem__(self, idx):
        return self._levels[idx]

    def back(self):
        return self._levels[-1]

    def clear(self):
        if self._h:
            self._L.vm_pyramid_destroy(self._h)
            self._h = None
        self._levels = []
        self._vector, self._qpath = [], []
        self._extends1, self._extends2 = [], []

    __del__ = clear

    def build_levels(self, sizes):
        """Allocate from explicit (w, h) level sizes, finest first."""
        self.clear()
        n = len(sizes)
        ws = (C.c_int * n)(*[int(s[0]) for s in sizes])
        hs = (C.c_int * n)(*[int(s[1]) for s in sizes])
        h = C.c_void_p()
        capi.check(self._L.vm_pyramid_create(self._ctx._h, n, ws, hs, C.byref(h)))
        self._h = h
        self._levels = [PyramidLevel(self, 0, sizes[0][0], sizes[0][1])]
        for k, (w, hh) in enumerate(sizes):
            self._levels.append(PyramidLevel(self, k + 1, w, hh))

    def upload_luma(self, el, img0, img1):
        img0 = np.ascontiguousarray(img0, dtype=np.float32)
        img1 = np.ascontiguousarray(img1, dtype=np.float32)
        lv = self._levels[el]
        assert img0.shape == (lv.height, lv.width) and img1.shape == img0.shape
        capi.check(self._L.vm_level_upload_luma(self._h, el - 1, img0.ctypes.data,
                                                img1.ctypes.data, 0))

    def build(self, img0, img1, start_res, nlevels=None):
        """Pyramid::build(video0, video1, ..., start_res), pyramid.cu:166-485, for
        one frame pair of float luma images.  Level geometry follows the
        reference (integer form of pyramid.cu:230-240, ceil halving :466-467);
        the images of the coarser levels come from a 2x2 box filter (the
        reference's Nehab-Hoppe B-spline prefiltered scale() is a 'next' row)."""
        h, w = img0.shape
        n = nlevels if nlevels is not None else synth.num_levels(w, h, start_res)
        n = max(n, 2)
        pyr = synth.build_pyramid(img0, img1, n)
        self.build_levels([(p[0].shape[1], p[0].shape[0]) for p in pyr])
        for k in range(n - 1):
            self.upload_luma(k + 1, pyr[k][0], pyr[k][1])
        self._vector = [np.zeros((h, w, 2), dtype=np.float32)]
        self._qpath = [np.zeros((h, w, 2), dtype=np.float32)]
        return pyr


def _pyramid_build_rgb(self, rgb0, rgb1, start_res, nlevels=None):
    """Pyramid::build for one pair of RGB8 frames with the reference's own image chain
    (pyramid.cu:203-211, 268-279, 355-364: load, Nehab-Hoppe cubic B-spline scale() per
    level, store_gray), run on the device (vm_pyramid.hip)."""
    rgb0 = np.ascontiguousarray(rgb0, dtype=np.uint8)
    rgb1 = np.ascontiguousarray(rgb1, dtype=np.uint8)
    h, w = rgb0.shape[:2]
    assert rgb0.shape == (h, w, 3) and rgb1.shape == rgb0.shape
    n = max(nlevels if nlevels is not None else synth.num_levels(w, h, start_res), 2)
    sizes = [(w, h)]
    for _ in range(n - 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    self.build_levels(sizes)
    capi.check(self._L.vm_pyramid_build_rgb(self._h, rgb0.ctypes.data, rgb1.ctypes.data, 0))
    self._vector = [np.zeros((h, w, 2), dtype=np.float32)]
    self._qpath = [np.zeros((h, w, 2), dtype=np.float32)]


Pyramid.build_rgb = _pyramid_build_rgb


class Morph(object):
    """class Morph, morph.h:10-31."""

    def __init__(self, params, pyramid, run_flag=None, fixed_work=False, keep_state=False):
        self.m_params, self.m_pyramid = params, pyramid
        # bool& run_flag of the reference: a shared int the caller may clear
        self.m_cb = run_flag if run_flag is not None else C.c_int(1)
        self.fixed_work = bool(fixed_work)
        # keep_state: skip the reference's clear_level (morph.cu:162) so that the error view of every level
        # (PyramidLevel.energy / error_map / error_image) can still be read after the solve
        self.keep_state = bool(keep_state)
        self.energies = {}   # level -> the five totals (PyramidLevel.energy()), filled as each level finishes
        # ctor, morph.cu:122-141
        self._total_l = pyramid.size() - 1
        self._current_l = self._total_l
        self._total_iter = self._current_iter = 0.0
        self._max_iter = float(params.max_iter)
        iter_num = int(params.max_iter)
        for el in range(self._total_l - 1, 0, -1):
            lv = pyramid[el]
            self._total_iter += iter_num * lv.width * lv.height * lv.depth
            iter_num = int(iter_num / params.max_iter_drop_factor)
        self.progress = {}

    def params(self):
        return self.m_params

    def calculate_halfway_parametrization(self):
        """morph.cu:150-168; returns True like the reference.  Raises VmError
        (the reference throws std::runtime_error from rod::check_cuda_error)."""
        P, pyr, L = self.m_params, self.m_pyramid, self.m_pyramid._L
        ctx = pyr._ctx
        ctx.set_params(KernParameters(P))
        cons, n = _cons_array(P.constraints(0))
        w0, h0 = pyr[0].width, pyr[0].height
        flag = C.cast(C.pointer(self.m_cb), C.c_void_p)
        capi.check(L.vm_coarse_solve(pyr._h, self._total_l - 1, w0, h0, cons, n))
        self._current_l = self._total_l - 1
        while self._current_l > 0:
            if self.m_cb.value:
                el = self._current_l
                capi.check(L.vm_upsample_v(pyr._h, el - 1, el))
                capi.check(L.vm_init_level(pyr._h, el - 1, w0, h0, cons, n))
                pr = capi.Progress()
                rc = L.vm_optimize_level(pyr._h, el - 1, self._max_iter, flag,
                                         int(self.fixed_work), C.byref(pr))
                if rc != capi.VM_E_CANCELLED:
                    capi.check(rc)
                lv = pyr[el]
                # morph.cu:1389-1391: the level is accounted as max_iter sweeps
                self._current_iter += lv.width * lv.height * self._max_iter
                self.progress[el] = dict(iters=pr.iters, iters_live=pr.iters_live, improving=pr.improving,
                                         pixel_iters=pr.pixel_iters, elapsed_ms=pr.elapsed_ms,
                                         launches=pr.launches, active_tiles=pr.active_tiles,
                                         candidates=pr.candidates, commits=pr.commits,
                                         evaluations=pr.evaluations,
                                         width=lv.width, height=lv.height)
                self.energies[el] = lv.energy()
                if not self.keep_state:
                    capi.check(L.vm_level_clear(pyr._h, el - 1))
                self._max_iter /= P.max_iter_drop_factor
            self._current_l -= 1
        return True


def solve_batch(pyramids, max_iter, max_iter_drop_factor=1.0, fixed_work=False, run_flag=None, constraints=None):
    """Morph::calculate_halfway_parametrization for a batch of frame pairs (same context,
    same geometry) in lockstep: vm_solve_batch / vm_solve_batch_cons.  constraints: None, one (n, 5) array of
    (lx, ly, rx, ry, weight) shared by every pair, or a list with one such array per pair.  Returns one list of
    per-level progress dicts (finest first) per pair."""
    n = len(pyramids)
    L = pyramids[0]._L
    nl = pyramids[0].size() - 2
    arr = (C.c_void_p * n)(*[p._h for p in pyramids])
    prog = (capi.Progress * (n * nl))()
    flag = C.cast(C.pointer(run_flag), C.c_void_p) if run_flag is not None else None
    if constraints is None:
        capi.check(L.vm_solve_batch(arr, n, float(max_iter), float(max_iter_drop_factor), flag,
                                    int(bool(fixed_work)), prog))
    else:
        per = constraints if isinstance(constraints, (list, tuple)) and len(constraints) == n and np.ndim(constraints[0]) == 2 else [constraints] * n
        keep = [_cons_array(c) for c in per]
        ptrs = (C.c_void_p * n)(*[C.cast(a, C.c_void_p).value for a, _ in keep])
        cnts = (C.c_int * n)(*[k for _, k in keep])
        capi.check(L.vm_solve_batch_cons(arr, n, float(max_iter), float(max_iter_drop_factor), ptrs, cnts, flag,
                                         int(bool(fixed_work)), prog))
    out = []
    for i in range(n):
        out.append([dict(iters=prog[i * nl + k].iters, iters_live=prog[i * nl + k].iters_live, improving=prog[i * nl + k].improving,
                         pixel_iters=prog[i * nl + k].pixel_iters, elapsed_ms=prog[i * nl + k].elapsed_ms,
                         launches=prog[i * nl + k].launches, commits=prog[i * nl + k].commits,
                         candidates=prog[i * nl + k].candidates, active_tiles=prog[i * nl + k].active_tiles,
                         evaluations=prog[i * nl + k].evaluations)
                    for k in range(nl)])
    return out


class _SolverThread(object):
    """What the reference's QThread subclasses (CMatchingThread, CSyncThread) share: the cancel flag the solver polls,
    percentage / run_time, a worker thread, and wait() re-raising what the worker met."""

    def __init__(self):
        self._flag = C.c_int(1)
        self.percentage = 0.0
        self.run_time = 0.0
        self._thread = None
        self.error = None

    @property
    def runflag(self):
        return bool(self._flag.value)

    @runflag.setter
    def runflag(self, v):
        self._flag.value = 1 if v else 0

    def _flag_ptr(self):
        """the flag as the C-ABI's `volatile const int *run_flag`"""
        return C.cast(C.pointer(self._flag), C.c_void_p)

    def run(self):
        """CMatchingThread::run / CSyncThread::run: _solve(), then update_result(); run_time is the solve's"""
        t0 = time.time()
        try:   # the whole body: an error of the delivery must reach wait() like one of the solve
            self._solve()
            self.run_time = time.time() - t0
            self.update_result()
        except Exception as e:  # surfaced to the caller of wait()
            self.error = e
            self.run_time = time.time() - t0

    def start(self):
        self._thread = threading.Thread(target=self.run)
        self._thread.start()

    def wait(self):
        if self._thread is not None:
            self._thread.join()
        if self.error is not None:
            raise self.error


class MatchingThread(_SolverThread):
    """class CMatchingThread, MatchingThread.h:7-37, on threading.Thread."""

    def __init__(self, parameters, pyramids, fixed_work=False, keep_state=False):
        _SolverThread.__init__(self)
        self._parameters, self._pyramids = parameters, pyramids
        self.gpu_morph = Morph(parameters, pyramids, self._flag, fixed_work, keep_state)

    @property
    def energies(self):
        """{level: the five energy totals}, one entry per level the solve has finished (Morph.energies)"""
        return self.gpu_morph.energies

    def _solve(self):
        """MatchingThread.cpp:138-150"""
        self.gpu_morph.calculate_halfway_parametrization()

    def update_result(self):
        """MatchingThread.cpp:22-84: fetch v of the current level, scale to full
        resolution and store it in pyramid._vector[0]."""
        pyr = self._pyramids
        el = max(self.gpu_morph._current_l, 1)
        w0, h0 = pyr[0].width, pyr[0].height
        out = np.zeros((h0, w0, 2), dtype=np.float32)
        capi.check(pyr._L.vm_upscale_result(pyr._h, el - 1, w0, h0, out.ctypes.data, 0))
        pyr._vector = [out]
        m = self.gpu_morph
        self.percentage = (m._current_iter / m._total_iter * 100.0) if m._total_iter else 100.0
        return out


class Frame(object):
    """Device-resident inputs of one output frame (vm_frame): the compositor
    side of RenderWidget::RenderStage2 and CPoissonExt."""

    def __init__(self, ctx, w, h, ex):
        self._ctx, self._L = ctx, capi.load()
        self.w, self.h, self.ex = int(w), int(h), int(ex)
        hh = C.c_void_p()
        capi.check(self._L.vm_frame_create(ctx._h, self.w, self.h, self.ex, C.byref(hh)))
        self._h = hh

    def close(self):
        if getattr(self, "_h", None):
            self._L.vm_frame_destroy(self._h)
            self._h = None

    __del__ = close

    def upload_rgb(self, rgb0, rgb1):
        """the two frames as (h, w, 3) uint8: the extended canvases are built on the device (Pyramid::build,
        pyramid.cu:186-200) -- vm_frame_upload_rgb; v and the quadratic path stay what they are"""
        a0, a1 = np.ascontiguousarray(rgb0, dtype=np.uint8), np.ascontiguousarray(rgb1, dtype=np.uint8)
        assert a0.shape == (self.h, self.w, 3) and a1.shape == a0.shape
        capi.check(self._L.vm_frame_upload_rgb(self._h, a0.ctypes.data, a1.ctypes.data, 0))

    def upload(self, ext0=None, ext1=None, v=None, qpath=None):
        def ptr(a, dt):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=dt)
            return a, a.ctypes.data
        cw, ch = self.w + 2 * self.ex, self.h + 2 * self.ex
        a0, p0 = ptr(ext0, np.uint8)
        a1, p1 = ptr(ext1, np.uint8)
        av, pv = ptr(v, np.float32)
        aq, pq = ptr(qpath, np.float32)
        for a in (a0, a1):
            assert a is None or a.shape == (ch, cw, 4)
        for a in (av, aq):
            assert a is None or a.shape == (self.h, self.w, 2)
        capi.check(self._L.vm_frame_upload(self._h, p0, p1, pv, pq))

    def set_v_from_level(self, pyramid, el):
        capi.check(self._L.vm_frame_set_v_from_level(self._h, pyramid._h, el - 1))

    def set_v_from_video(self, video, lvl, frame):
        """frame `frame` of CMatchingThread::update_result over a video pair, left in this frame's v on
        the device (the frame's size is the result's w0 x h0)"""
        capi.check(self._L.vm_frame_set_v_from_video(self._h, video._h, int(lvl), int(frame)))

    def download_ext(self, side):
        out = np.zeros((self.h + 2 * self.ex, self.w + 2 * self.ex, 4), dtype=np.uint8)
        capi.check(self._L.vm_frame_download_ext(self._h, side, out.ctypes.data))
        return out

    def _render(self, name, args, grid, layers, vp=None):
        """one downloading vm_render_* call (after the handle: the viewport, if the call takes one, then args) into a host
        array over grid = (rows, columns): uint8 RGB, or float32 with the channels the layers were uploaded in"""
        if layers:
            shape = getattr(self, "_layer_shape", (self.h, self.w))       # (no upload: the call answers VM_E_STATE)
            out = np.empty(tuple(grid) + tuple(shape[2:]), dtype=np.float32)
        else:
            out = np.zeros(tuple(grid) + (3,), dtype=np.uint8)
        head = () if vp is None else (C.byref(vp),)
        capi.check(getattr(self._L, name)(self._h, *head, *args, out.ctypes.data, 0))
        return out

    def _render_dev(self, name, args, vp=None):
        """the same call's _dev twin: the output stays on the device, the launch's milliseconds come back"""
        ms = C.c_float(0)
        head = () if vp is None else (C.byref(vp),)
        capi.check(getattr(self._L, name)(self._h, *head, *args, C.byref(ms)))
        return ms.value

    def render_halfway(self, color_fa, geo_fa, color_from):
        """render_halfway_image, render.cu:62-96 -> (h, w, 3) uint8."""
        return self._render("vm_render_halfway", (color_fa, geo_fa, color_from), (self.h, self.w), False)

    def render_halfway_dev(self, color_fa, geo_fa, color_from):
        return self._render_dev("vm_render_halfway_dev", (color_fa, geo_fa, color_from))

    def sampling_maps(self, geo_fa):
        """where every output pixel of render_halfway at geo_fa samples image 0 and image 1, and how well that is
        founded (vm_frame_sampling_maps): (map0 (h, w, 2) float32, map1 (h, w, 2) float32, resid (h, w) float32 -- the
        move of the fixed point's last round --, flags (h, w) uint8 -- bit 0 / 1: map0 / map1 inside the image).  At
        geo_fa = 0 map1 is the forward map image 0 -> image 1, at geo_fa = 1 map0 the backward map."""
        m0 = np.empty((self.h, self.w, 2), dtype=np.float32)
        m1 = np.empty((self.h, self.w, 2), dtype=np.float32)
        resid = np.empty((self.h, self.w), dtype=np.float32)
        flags = np.empty((self.h, self.w), dtype=np.uint8)
        capi.check(self._L.vm_frame_sampling_maps(self._h, float(geo_fa), m0.ctypes.data, m1.ctypes.data,
                                                  resid.ctypes.data, flags.ctypes.data))
        return m0, m1, resid, flags

    def upload_layers(self, l0, l1):
        """two float32 layers, (h, w) or (h, w, C) with C in 1..4 (a matte, a depth or UV pass, a float plate), kept on
        the device for render_layers (vm_frame_upload_layers); uploading again replaces them"""
        a0, a1 = np.ascontiguousarray(l0, dtype=np.float32), np.ascontiguousarray(l1, dtype=np.float32)
        assert a0.shape == a1.shape and a0.shape[:2] == (self.h, self.w) and a0.ndim in (2, 3)
        self._layer_shape = a0.shape
        capi.check(self._L.vm_frame_upload_layers(self._h, 1 if a0.ndim == 2 else a0.shape[2], a0.ctypes.data, a1.ctypes.data, 0))

    def extend_layers(self, tol=1e-5, max_it=20000):
        """the uploaded layers extended past the image edge as the canvases are (vm_frame_extend_layers;
        PoissonExt.cpp:49-362): from then on every layer render call samples the extension instead of repeating the
        edge texel.  A new upload_layers drops it.  Returns ([((iters, rel) side 1, (iters, rel) side 2) per group of up
        to three channels], elapsed ms)."""
        shape = getattr(self, "_layer_shape", (self.h, self.w))           # (no upload: the call answers VM_E_STATE)
        n = ((shape[2] if len(shape) == 3 else 1) + 2) // 3
        it, rr, ms = (C.c_int * (2 * n))(), (C.c_float * (2 * n))(), C.c_float(0)
        capi.check(self._L.vm_frame_extend_layers(self._h, float(tol), int(max_it), it, rr, C.byref(ms)))
        return [((it[2 * g], rr[2 * g]), (it[2 * g + 1], rr[2 * g + 1])) for g in range(n)], ms.value

    def download_layers_ext(self, side):
        """the extended layer of side 1 or 2 (vm_frame_download_layers_ext): float32 (h + 2 ex, w + 2 ex) with the
        channels the layers were uploaded in"""
        shape = getattr(self, "_layer_shape", (self.h, self.w))
        out = np.empty((self.h + 2 * self.ex, self.w + 2 * self.ex) + tuple(shape[2:]), dtype=np.float32)
        capi.check(self._L.vm_frame_download_layers_ext(self._h, int(side), out.ctypes.data, 0))
        return out

    def drop_layer_extension(self):
        """back to the tight layers (vm_frame_drop_layer_extension)"""
        capi.check(self._L.vm_frame_drop_layer_extension(self._h))

    def layers_prepare(self, side):
        """diagnostic (vm_dbg_layers_prepare): what the extension of one side solves, before any solve -- (filled canvas,
        valid, type map, right-hand side); the frame is not changed"""
        shape = getattr(self, "_layer_shape", (self.h, self.w))
        grid = (self.h + 2 * self.ex, self.w + 2 * self.ex)
        filled = np.empty(grid + tuple(shape[2:]), dtype=np.float32)
        rhs = np.empty_like(filled)
        valid, typ = np.empty(grid, dtype=np.uint8), np.empty(grid, dtype=np.uint8)
        capi.check(self._L.vm_dbg_layers_prepare(self._h, int(side), filled.ctypes.data, valid.ctypes.data, typ.ctypes.data,
                                                 rhs.ctypes.data))
        return filled, valid, typ, rhs

    def render_layers(self, color_fa, geo_fa, color_from):
        """the uploaded layers through the morph (vm_render_layers): float32 of the shape they were uploaded in"""
        return self._render("vm_render_layers", (color_fa, geo_fa, color_from), (self.h, self.w), True)

    def render_layers_dev(self, color_fa, geo_fa, color_from):
        return self._render_dev("vm_render_layers_dev", (color_fa, geo_fa, color_from))

    def upload_schedule(self, geo=None, color=None):
        """the transition schedule (vm_frame_upload_schedule): (h, w, 2) float32 planes of (t0, t1) in the halfway
        domain for the geometry and the colour (videomorphing_amd.transition builds them); one of them may be None:
        uniform (0, 1).  Uploading again replaces the schedule."""
        def ptr(a):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=np.float32)
            assert a.shape == (self.h, self.w, 2)
            return a, a.ctypes.data
        ag, pg = ptr(geo)
        ac, pc = ptr(color)
        capi.check(self._L.vm_frame_upload_schedule(self._h, pg, pc, 0))

    def clear_schedule(self):
        capi.check(self._L.vm_frame_clear_schedule(self._h))

    def render_transition(self, t, ease=capi.EASE_LINEAR, color_from=1):
        """render_halfway under the schedule at time t (vm_render_transition) -> (h, w, 3) uint8"""
        return self._render("vm_render_transition", (float(t), int(ease), int(color_from)), (self.h, self.w), False)

    def render_transition_dev(self, t, ease=capi.EASE_LINEAR, color_from=1):
        return self._render_dev("vm_render_transition_dev", (float(t), int(ease), int(color_from)))

    def render_transition_layers(self, t, ease=capi.EASE_LINEAR, color_from=1):
        """the uploaded layers under the schedule at time t (vm_render_transition_layers): float32 of the shape they
        were uploaded in"""
        return self._render("vm_render_transition_layers", (float(t), int(ease), int(color_from)), (self.h, self.w), True)

    def render_transition_layers_dev(self, t, ease=capi.EASE_LINEAR, color_from=1):
        return self._render_dev("vm_render_transition_layers_dev", (float(t), int(ease), int(color_from)))

    def transition_maps(self, t, ease=capi.EASE_LINEAR):
        """sampling_maps under the schedule at time t (vm_frame_transition_maps): (map0, map1, resid, flags, rates) --
        rates (h, w, 2) float32: the geometric and the colour rate (g, k) of every output pixel after the last round"""
        m0 = np.empty((self.h, self.w, 2), dtype=np.float32)
        m1 = np.empty((self.h, self.w, 2), dtype=np.float32)
        resid = np.empty((self.h, self.w), dtype=np.float32)
        flags = np.empty((self.h, self.w), dtype=np.uint8)
        rates = np.empty((self.h, self.w, 2), dtype=np.float32)
        capi.check(self._L.vm_frame_transition_maps(self._h, float(t), int(ease), m0.ctypes.data, m1.ctypes.data,
                                                    resid.ctypes.data, flags.ctypes.data, rates.ctypes.data))
        return m0, m1, resid, flags, rates

    def _carry(self, name, head, points, times, want=None, timed=False):
        """one vm_frame_carry_points* call: points (n, 2) (or (2,)) float32 of the output frame at the from-time, carried to
        `times` -> (out (nt, n, 2), halfway, pos0, pos1 (n, 2), resid (n,) float32, flags (n,) uint8); `want` names the
        outputs to ask for (the others come back None); timed: the launch's milliseconds are appended"""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        to = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float32)
        n, nt = len(pts), len(to)
        names = ("out", "halfway", "pos0", "pos1", "resid", "flags")
        shapes = ((nt, n, 2), (n, 2), (n, 2), (n, 2), (n,), (n,))
        outs = [np.empty(s, dtype=np.uint8 if k == "flags" else np.float32) if want is None or k in want else None
                for k, s in zip(names, shapes)]
        ms = C.c_float(0)
        capi.check(getattr(self._L, name)(self._h, *head, pts.ctypes.data, n, to.ctypes.data, nt,
                                          *[None if a is None else a.ctypes.data for a in outs], C.byref(ms) if timed else None))
        return tuple(outs) + ((ms.value,) if timed else ())

    def carry_points(self, points, from_fa, to_fa, want=None, timed=False):
        """where the points (n, 2) of the output frame at geo_fa = from_fa lie at every time of to_fa
        (vm_frame_carry_points; image 0 is time 0, image 1 time 1, pixel centre i is i): (out (nt, n, 2), halfway, pos0,
        pos1 (n, 2), resid (n,), flags (n,)) -- the position at each to-time, in the halfway domain, in image 0 and in
        image 1, the move of the chain's last round, bit 0 / 1: pos0 / pos1 inside the image"""
        return self._carry("vm_frame_carry_points", (float(from_fa),), points, to_fa, want, timed)

    def carry_points_transition(self, points, t_from, t_to, ease=capi.EASE_LINEAR, want=None, timed=False):
        """carry_points under the schedule (vm_frame_carry_points_transition): the from-time and the to-times are times
        of the schedule"""
        return self._carry("vm_frame_carry_points_transition", (float(t_from), int(ease)), points, t_to, want, timed)

    def _motion(self, name, head, times, want):
        to = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float32)
        names = ("out", "resid", "flags")
        shapes = ((len(to), self.h, self.w, 2), (self.h, self.w), (self.h, self.w))
        outs = [np.empty(s, dtype=np.uint8 if k == "flags" else np.float32) if want is None or k in want else None
                for k, s in zip(names, shapes)]
        capi.check(getattr(self._L, name)(self._h, *head, to.ctypes.data, len(to),
                                          *[None if a is None else a.ctypes.data for a in outs]))
        return tuple(outs)

    def _motion_dev(self, name, head, times):
        to = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float32)
        ms = C.c_float(0)
        capi.check(getattr(self._L, name)(self._h, *head, to.ctypes.data, len(to), C.byref(ms)))
        return ms.value

    def motion_maps(self, from_fa, to_fa, want=None):
        """carry_points from every pixel centre of the output frame at from_fa (vm_frame_motion_maps): (out
        (nt, h, w, 2), resid (h, w), flags (h, w)); out[k] minus the pixel grid is the motion-vector pass to time
        to_fa[k].  At most 16 to-times."""
        return self._motion("vm_frame_motion_maps", (float(from_fa),), to_fa, want)

    def motion_maps_dev(self, from_fa, to_fa):
        return self._motion_dev("vm_frame_motion_maps_dev", (float(from_fa),), to_fa)

    def transition_motion_maps(self, t_from, t_to, ease=capi.EASE_LINEAR, want=None):
        """motion_maps under the schedule (vm_frame_transition_motion_maps)"""
        return self._motion("vm_frame_transition_motion_maps", (float(t_from), int(ease)), t_to, want)

    def transition_motion_maps_dev(self, t_from, t_to, ease=capi.EASE_LINEAR):
        return self._motion_dev("vm_frame_transition_motion_maps_dev", (float(t_from), int(ease)), t_to)

    def constraint_gaps(self, constraints):
        """how well each constraint is met, in pixels: rows (lx, ly, rx, ry[, weight]) or capi.Constraint items.  (lx, ly)
        carried from image 0 gives pos1, compared with (rx, ry); (rx, ry) carried from image 1 gives pos0, compared with
        (lx, ly) -> (gap01, gap10, resid01, resid10), one float32 per row each (a resid that is not small says the chain
        had not settled there, and the gap beside it means little); no constraints: four empty arrays"""
        if len(constraints) and isinstance(constraints[0], capi.Constraint):
            constraints = [(c.lx, c.ly, c.rx, c.ry) for c in constraints]
        if not len(constraints):
            return tuple(np.empty(0, np.float32) for _ in range(4))
        c = np.asarray(constraints, dtype=np.float32).reshape(len(constraints), -1)[:, :4]
        _, _, _, p1, r01, _ = self.carry_points(c[:, 0:2], 0.0, [1.0], want=("pos1", "resid"))
        _, _, p0, _, r10, _ = self.carry_points(c[:, 2:4], 1.0, [0.0], want=("pos0", "resid"))
        gap01 = np.hypot(p1[:, 0] - c[:, 2], p1[:, 1] - c[:, 3])
        gap10 = np.hypot(p0[:, 0] - c[:, 0], p0[:, 1] - c[:, 1])
        return gap01, gap10, r01, r10

    @staticmethod
    def _shutter_args(color_fa, geo_open, geo_close, samples, color_from):
        return (float(color_fa), float(geo_open), float(geo_close), int(samples), int(color_from))

    def render_shutter(self, color_fa, geo_open, geo_close, samples, color_from=1):
        """render_halfway with motion blur (vm_render_shutter): the mean over `samples` (1..64) times between geo_open
        and geo_close, each clamped to [0, 1], taken in float32 before the one rounding -> (h, w, 3) uint8"""
        args = self._shutter_args(color_fa, geo_open, geo_close, samples, color_from)
        return self._render("vm_render_shutter", args, (self.h, self.w), False)

    def render_shutter_dev(self, color_fa, geo_open, geo_close, samples, color_from=1):
        return self._render_dev("vm_render_shutter_dev", self._shutter_args(color_fa, geo_open, geo_close, samples, color_from))

    def render_shutter_layers(self, color_fa, geo_open, geo_close, samples, color_from=1):
        """the uploaded layers through the same shutter (vm_render_shutter_layers): float32 of the shape they were
        uploaded in -- a matte blurs exactly as its plate does"""
        args = self._shutter_args(color_fa, geo_open, geo_close, samples, color_from)
        return self._render("vm_render_shutter_layers", args, (self.h, self.w), True)

    def render_shutter_layers_dev(self, color_fa, geo_open, geo_close, samples, color_from=1):
        return self._render_dev("vm_render_shutter_layers_dev", self._shutter_args(color_fa, geo_open, geo_close, samples, color_from))

    @staticmethod
    def _viewport_grid(s):
        """(out_h, out_w) of a vm_viewport; one the library will refuse gets a buffer of one pixel"""
        ok = 1 <= s.out_w <= 32768 and 1 <= s.out_h <= 32768
        return (s.out_h, s.out_w) if ok else (1, 1)

    def render_viewport(self, vp, color_fa, geo_fa, color_from=1):
        """render_halfway through a viewport (vm_render_viewport; vp: a videomorphing_amd.viewport.Viewport): any window
        of the morph at any size, every output pixel the mean of vp.nx x vp.ny chains taken in float32 before the one
        rounding -> (vp.out_h, vp.out_w, 3) uint8.  The library checks the viewport (VmError, VM_E_INVALID)."""
        s = vp.struct()
        return self._render("vm_render_viewport", (float(color_fa), float(geo_fa), int(color_from)), self._viewport_grid(s), False, s)

    def render_viewport_dev(self, vp, color_fa, geo_fa, color_from=1):
        return self._render_dev("vm_render_viewport_dev", (float(color_fa), float(geo_fa), int(color_from)), vp.struct())

    def render_viewport_layers(self, vp, color_fa, geo_fa, color_from=1):
        """the uploaded layers through the same viewport (vm_render_viewport_layers): float32 (vp.out_h, vp.out_w) or
        (vp.out_h, vp.out_w, C) as they were uploaded -- a matte is filtered exactly as its plate is"""
        s = vp.struct()
        return self._render("vm_render_viewport_layers", (float(color_fa), float(geo_fa), int(color_from)), self._viewport_grid(s), True, s)

    def render_viewport_layers_dev(self, vp, color_fa, geo_fa, color_from=1):
        return self._render_dev("vm_render_viewport_layers_dev", (float(color_fa), float(geo_fa), int(color_from)), vp.struct())

    def render_viewport_filtered(self, vp, filter, color_fa, geo_fa, color_from=1):
        """render_viewport with a cubic filter on the taps that read the canvases (vm_frame_render_viewport_filtered; filter: a
        capi.FILTER_*): Catmull-Rom, Mitchell or the cubic B-spline over 4 x 4 texels, the mean clamped to [0, 255] before
        the rounding -> (vp.out_h, vp.out_w, 3) uint8.  FILTER_BILINEAR is render_viewport, bit for bit."""
        s = vp.struct()
        args = (int(filter), float(color_fa), float(geo_fa), int(color_from))
        return self._render("vm_frame_render_viewport_filtered", args, self._viewport_grid(s), False, s)

    def render_viewport_filtered_dev(self, vp, filter, color_fa, geo_fa, color_from=1):
        return self._render_dev("vm_frame_render_viewport_filtered_dev", (int(filter), float(color_fa), float(geo_fa), int(color_from)), vp.struct())

    def render_viewport_filtered_layers(self, vp, filter, color_fa, geo_fa, color_from=1):
        """the uploaded layers through the same viewport and filter (vm_frame_render_viewport_filtered_layers): float32 as
        render_viewport_layers gives them, NOT clamped -- a cubic filter overshoots, and a matte may leave [0, 1]"""
        s = vp.struct()
        args = (int(filter), float(color_fa), float(geo_fa), int(color_from))
        return self._render("vm_frame_render_viewport_filtered_layers", args, self._viewport_grid(s), True, s)

    def render_viewport_filtered_layers_dev(self, vp, filter, color_fa, geo_fa, color_from=1):
        return self._render_dev("vm_frame_render_viewport_filtered_layers_dev", (int(filter), float(color_fa), float(geo_fa), int(color_from)), vp.struct())

    def _multiband(self, name, bands, args, layers):
        """one multiband call or its _dev twin (bands: a videomorphing_amd.multiband.Bands; the library checks it); what the
        call blended is kept for multiband_level"""
        s = bands.struct()
        if name.endswith("_dev"):
            out = self._render_dev(name, args, s)
        else:
            out = self._render(name, args, (self.h, self.w), layers, s)
        self._mb_tail = tuple(getattr(self, "_layer_shape", (self.h, self.w))[2:]) if layers else (3,)
        self._mb_layers = layers
        return out

    def render_multiband(self, bands, color_fa, geo_fa):
        """render_halfway's blend (color_from = 1) band by band (vm_frame_render_multiband): the two warped plates and the
        weight color_fa split into bands.levels + 1 frequency bands, every band blended under its level's weight plane
        sharpened by bands.sharp[l], the sum clamped to [0, 255] before the rounding -> (h, w, 3) uint8"""
        return self._multiband("vm_frame_render_multiband", bands, (float(color_fa), float(geo_fa)), False)

    def render_multiband_dev(self, bands, color_fa, geo_fa):
        return self._multiband("vm_frame_render_multiband_dev", bands, (float(color_fa), float(geo_fa)), False)

    def render_multiband_layers(self, bands, color_fa, geo_fa):
        """the uploaded layers under the same bands (vm_frame_render_multiband_layers): float32 of the shape they were
        uploaded in, neither clamped nor rounded"""
        return self._multiband("vm_frame_render_multiband_layers", bands, (float(color_fa), float(geo_fa)), True)

    def render_multiband_layers_dev(self, bands, color_fa, geo_fa):
        return self._multiband("vm_frame_render_multiband_layers_dev", bands, (float(color_fa), float(geo_fa)), True)

    def render_multiband_transition(self, bands, t, ease=capi.EASE_LINEAR):
        """render_transition's blend band by band (vm_frame_render_multiband_transition): the colour rate k of every output
        pixel is the weight the bands smooth, so a wipe's seam is wide in the low frequencies and narrow in the detail"""
        return self._multiband("vm_frame_render_multiband_transition", bands, (float(t), int(ease)), False)

    def render_multiband_transition_dev(self, bands, t, ease=capi.EASE_LINEAR):
        return self._multiband("vm_frame_render_multiband_transition_dev", bands, (float(t), int(ease)), False)

    def render_multiband_transition_layers(self, bands, t, ease=capi.EASE_LINEAR):
        return self._multiband("vm_frame_render_multiband_transition_layers", bands, (float(t), int(ease)), True)

    def render_multiband_transition_layers_dev(self, bands, t, ease=capi.EASE_LINEAR):
        return self._multiband("vm_frame_render_multiband_transition_layers_dev", bands, (float(t), int(ease)), True)

    def multiband_level(self, what, level):
        """diagnostic (vm_dbg_multiband_level): one level of what this frame's last multiband call left -- what: capi.MB_G0,
        MB_G1 (the Gaussian levels of the two plates), MB_MASK (the weight plane before sharpening), MB_OUT (the sum of the
        bands from the coarsest down to this level; level 0 after a layers call only) -> float32 (h_l, w_l, C), C = 3
        after an RGB8 call, the layers' shape after a layer call; (h_l, w_l) for the mask"""
        w, h = self.w, self.h
        for _ in range(max(0, min(int(level), capi.MULTIBAND_MAX_LEVELS))):
            w, h = (w + 1) // 2, (h + 1) // 2
        tail = () if what == capi.MB_MASK else getattr(self, "_mb_tail", (3,))
        buf = np.empty(h * w * 4, dtype=np.float32)        # (room for four channels whatever the last call blended)
        capi.check(self._L.vm_dbg_multiband_level(self._h, int(what), int(level), buf.ctypes.data))
        return buf[:h * w * int(np.prod(tail, dtype=np.int64))].reshape((h, w) + tail).copy()

    def render_viewport_shutter(self, vp, color_fa, geo_open, geo_close, samples, color_from=1):
        """render_viewport with motion blur (vm_render_viewport_shutter): every output pixel the mean of its vp.nx x vp.ny
        chains at each of `samples` (1..64) times between geo_open and geo_close, each clamped to [0, 1], taken in float32
        before the one rounding -> (vp.out_h, vp.out_w, 3) uint8.  samples * vp.nx * vp.ny may be 256 at most; the library
        checks that and the viewport (VmError, VM_E_INVALID)."""
        s, args = vp.struct(), self._shutter_args(color_fa, geo_open, geo_close, samples, color_from)
        return self._render("vm_render_viewport_shutter", args, self._viewport_grid(s), False, s)

    def render_viewport_shutter_dev(self, vp, color_fa, geo_open, geo_close, samples, color_from=1):
        args = self._shutter_args(color_fa, geo_open, geo_close, samples, color_from)
        return self._render_dev("vm_render_viewport_shutter_dev", args, vp.struct())

    def render_viewport_shutter_layers(self, vp, color_fa, geo_open, geo_close, samples, color_from=1):
        """the uploaded layers through the same viewport over the same shutter (vm_render_viewport_shutter_layers):
        float32 (vp.out_h, vp.out_w) or (vp.out_h, vp.out_w, C) as they were uploaded"""
        s, args = vp.struct(), self._shutter_args(color_fa, geo_open, geo_close, samples, color_from)
        return self._render("vm_render_viewport_shutter_layers", args, self._viewport_grid(s), True, s)

    def render_viewport_shutter_layers_dev(self, vp, color_fa, geo_open, geo_close, samples, color_from=1):
        args = self._shutter_args(color_fa, geo_open, geo_close, samples, color_from)
        return self._render_dev("vm_render_viewport_shutter_layers_dev", args, vp.struct())

    @staticmethod
    def _shutter_color_time(t_open, t_close, t_color):
        """t_color of the transition shutter calls; None: the float32 midpoint (t_open + t_close) * 0.5, formed here"""
        if t_color is not None:
            return float(t_color)
        return float((np.float32(t_open) + np.float32(t_close)) * np.float32(0.5))

    def _scheduled_args(self, t_open, t_close, samples, t_color, ease, color_from):
        tc = self._shutter_color_time(t_open, t_close, t_color)
        return (float(t_open), float(t_close), int(samples), tc, int(ease), int(color_from))

    def render_viewport_transition_shutter(self, vp, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR, color_from=1):
        """render_transition_shutter through a viewport (vm_render_viewport_transition_shutter): the geometry schedule
        ramped at each of `samples` times between t_open and t_close, the colour schedule once at t_color (None: the
        float32 midpoint, formed on the host), from the vp.nx x vp.ny sub-sample points of every output pixel ->
        (vp.out_h, vp.out_w, 3) uint8"""
        s, args = vp.struct(), self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render("vm_render_viewport_transition_shutter", args, self._viewport_grid(s), False, s)

    def render_viewport_transition_shutter_dev(self, vp, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR, color_from=1):
        args = self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render_dev("vm_render_viewport_transition_shutter_dev", args, vp.struct())

    def render_viewport_transition_shutter_layers(self, vp, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR,
                                                  color_from=1):
        """the uploaded layers through the same viewport, shutter and rates (vm_render_viewport_transition_shutter_layers)"""
        s, args = vp.struct(), self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render("vm_render_viewport_transition_shutter_layers", args, self._viewport_grid(s), True, s)

    def render_viewport_transition_shutter_layers_dev(self, vp, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR,
                                                      color_from=1):
        args = self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render_dev("vm_render_viewport_transition_shutter_layers_dev", args, vp.struct())

    def render_viewport_transition(self, vp, t, ease=capi.EASE_LINEAR, color_from=1):
        """render_transition through a viewport: the frame under its schedule at the one instant t, which is
        render_viewport_transition_shutter with samples = 1 and t_open == t_close == t_color == t"""
        return self.render_viewport_transition_shutter(vp, t, t, 1, t, ease, color_from)

    def render_transition_shutter(self, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR, color_from=1):
        """render_transition with motion blur (vm_render_transition_shutter): the mean over `samples` (1..64) times
        between t_open and t_close, the geometry schedule ramped at each of them, the colour schedule once at t_color
        (None: the float32 midpoint (t_open + t_close) * 0.5, formed on the host) -> (h, w, 3) uint8"""
        args = self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render("vm_render_transition_shutter", args, (self.h, self.w), False)

    def render_transition_shutter_dev(self, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR, color_from=1):
        args = self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render_dev("vm_render_transition_shutter_dev", args)

    def render_transition_shutter_layers(self, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR, color_from=1):
        """the uploaded layers through the same shutter under the schedule (vm_render_transition_shutter_layers): float32
        of the shape they were uploaded in; t_color None: the float32 midpoint, as above"""
        args = self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render("vm_render_transition_shutter_layers", args, (self.h, self.w), True)

    def render_transition_shutter_layers_dev(self, t_open, t_close, samples, t_color=None, ease=capi.EASE_LINEAR, color_from=1):
        args = self._scheduled_args(t_open, t_close, samples, t_color, ease, color_from)
        return self._render_dev("vm_render_transition_shutter_layers_dev", args)

    def quadratic_path(self, tol=1e-4, max_it=200):
        """CQuadraticPath::optimize for this frame's v (QuadraticPath.cpp:24-223); the result
        stays in the frame for render_halfway.  Returns (iterations, residual, ms)."""
        it, rr, ms = C.c_int(0), C.c_float(0), C.c_float(0)
        capi.check(self._L.vm_frame_quadratic_path(self._h, float(tol), int(max_it), C.byref(it), C.byref(rr), C.byref(ms)))
        return it.value, rr.value, ms.value

    def download_v(self):
        out = np.empty((self.h, self.w, 2), dtype=np.float32)
        capi.check(self._L.vm_frame_download_v(self._h, out.ctypes.data))
        return out

    def download_qpath(self):
        out = np.empty((self.h, self.w, 2), dtype=np.float32)
        capi.check(self._L.vm_frame_download_qpath(self._h, out.ctypes.data))
        return out

    def poisson_extend(self, side, tol=1e-5, max_it=20000):
        """CPoissonExt::prepare + poissonExtend for one side (PoissonExt.cpp:19-41)."""
        it, rr, ms = C.c_int(0), C.c_float(0), C.c_float(0)
        capi.check(self._L.vm_poisson_extend(self._h, side, tol, max_it, C.byref(it),
                                             C.byref(rr), C.byref(ms)))
        return it.value, rr.value, ms.value

    def poisson_extend_both(self, tol=1e-5, max_it=20000):
        """both sides of this frame as one batch: ((iters1, rel1), (iters2, rel2), ms)"""
        per_frame, ms = poisson_extend_frames([self], tol, max_it)
        return per_frame[0][0], per_frame[0][1], ms


def poisson_extend_frames(frames, tol=1e-5, max_it=20000):
    """CPoissonExt::run's loop body (PoissonExt.cpp:24-36) for several frames of one context at once: both sides of
    every frame are independent systems and share every launch.  Returns ([((iters, rel) side 1, (iters, rel) side 2)
    per frame], elapsed ms)."""
    n = len(frames)
    arr = (C.c_void_p * n)(*[f._h for f in frames])
    it, rr, ms = (C.c_int * (2 * n))(), (C.c_float * (2 * n))(), C.c_float(0)
    capi.check(frames[0]._L.vm_poisson_extend_frames(arr, n, tol, max_it, it, rr, C.byref(ms)))
    return [((it[2 * i], rr[2 * i]), (it[2 * i + 1], rr[2 * i + 1])) for i in range(n)], ms.value


def context_beside(device, math_mode, others, tries=8):
    """A new Context whose stream runs side by side with the streams of all `others` (contexts of the same device): the
    runtime deals new streams to its GPU_MAX_HW_QUEUES hardware queues as it likes, and two streams on one queue run their
    kernels one after the other.  Candidates that share a queue with one of `others` are kept alive while the search goes on
    (so that the next stream gets another queue) and closed at the end; after `tries` candidates the last one is returned
    whatever it shares.  The new context takes the reduction mode of others[0].  Returns (context, number of rejected
    candidates)."""
    rejected = []
    probe = not os.environ.get("VM_NO_STREAM_PROBE")          # development switch: take the first stream, as rounds 1-5 did
    while True:
        c = Context(device, math_mode)
        if others and others[0].reduction != c.reduction:
            c.set_reduction(others[0].reduction)
        if not probe or len(rejected) >= tries - 1 or all(c.runs_beside(o) for o in others):
            for r in rejected:
                r.close()
            return c, len(rejected)
        rejected.append(c)


def pin_host(array):
    """page-lock a numpy array frames are uploaded from (vm_host_register); returns the array"""
    a = np.ascontiguousarray(array)
    capi.check(capi.load().vm_host_register(a.ctypes.data, a.nbytes))
    return a


def unpin_host(array):
    capi.check(capi.load().vm_host_unregister(array.ctypes.data))


def make_extended(rgb, ex):
    """Extended RGBA8 canvas of Pyramid::build, pyramid.cu:186-200: filled with
    (255,255,255,255), the image pasted at (ex,ex) with alpha 0."""
    h, w = rgb.shape[:2]
    can = np.full((h + 2 * ex, w + 2 * ex, 4), 255, dtype=np.uint8)
    can[ex:ex + h, ex:ex + w, :3] = rgb
    can[ex:ex + h, ex:ex + w, 3] = 0
    return can


# ---------------------------------------------------------------------------------------------
# video pairs: class Pyramid with depth > 1 and the temporally coupled Morph

def _vcons_array(cons):
    """rows (lx, ly, rx, ry, weight, frame) -> VideoConstraint array"""
    cons = np.asarray(cons if cons is not None else [], dtype=np.float32).reshape(-1, 6)
    n = len(cons)
    arr = (capi.VideoConstraint * max(n, 1))()
    for k in range(n):
        arr[k] = capi.VideoConstraint(float(cons[k][0]), float(cons[k][1]), float(cons[k][2]), float(cons[k][3]),
                                      float(cons[k][4]), int(cons[k][5]))
    return arr, n


def video_constraints(P):
    """Parameters::lp/rp/cnt resolved with the frame of the left point (morph.cu:354-366)"""
    out = []
    for row in P.cnt:
        for c in row:
            l = P.lp[c.li[0]][c.li[1]]
            r = P.rp[c.ri[0]][c.ri[1]]
            out.append((l.p[0], l.p[1], r.p[0], r.p[1], min(l.weight, r.weight), l.p[2]))
    return np.asarray(out, dtype=np.float32).reshape(-1, 6)


class VideoPage(_ErrorView):
    """One page of a PyramidLevel of depth > 1 (device-state access)."""

    def __init__(self, vid, lvl, page, w, h):
        self._vid_ref, self._lvl, self._page = weakref.ref(vid), lvl, page   # no cycle (see PyramidLevel)
        self.width, self.height = int(w), int(h)

    @property
    def _vid(self):
        v = self._vid_ref()
        if v is None:
            raise capi.VmError(capi.VM_E_STATE, "this VideoPage outlived its VideoPyramid: keep a reference to the "
                                                "VideoPyramid while its pages are in use")
        return v

    def _err(self, name):
        return getattr(self._vid._L, "vm_video_" + name), (self._vid._h, self._lvl, self._page)

    def field(self, name):
        fid, ch = capi.FIELDS[name]
        if name == "impmask":
            out = np.zeros(((self.height + 4) // 5 + 2, (self.width + 4) // 5 + 2), dtype=np.uint32)
        elif ch == 2:
            out = np.zeros((self.height, self.width, 2), dtype=np.float32)
        else:
            out = np.zeros((self.height, self.width), dtype=np.float32)
        capi.check(self._vid._L.vm_video_get_field(self._vid._h, self._lvl, self._page, fid, out.ctypes.data))
        return out

    @property
    def v(self):
        out = np.zeros((self.height, self.width, 2), dtype=np.float32)
        capi.check(self._vid._L.vm_video_get_v(self._vid._h, self._lvl, self._page, out.ctypes.data, 0))
        return out

    @v.setter
    def v(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        assert arr.shape == (self.height, self.width, 2)
        capi.check(self._vid._L.vm_video_set_v(self._vid._h, self._lvl, self._page, arr.ctypes.data, 0))


class VideoPyramid(object):
    """class Pyramid (Pyramid.h:14-48) for a video pair: level l holds depth[l] pages and four
    flow fields per page.  pages[l][t]: l = 0 finest ... last = coarsest (v only)."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, capi.load()
        self._h = None
        self.levels, self.factor_t, self.pages = [], [], []

    def clear(self):
        if getattr(self, "_h", None):
            self._L.vm_video_destroy(self._h)
            self._h = None

    __del__ = clear

    def build_levels(self, levels, factor_t=None, depth0=None):
        """levels: [(w, h, d), ...] finest first incl. the coarsest"""
        self.clear()
        n = len(levels)
        ws = (C.c_int * n)(*[int(l[0]) for l in levels])
        hs = (C.c_int * n)(*[int(l[1]) for l in levels])
        ds = (C.c_int * n)(*[int(l[2]) for l in levels])
        ft = (C.c_int * n)(*[int(x) for x in factor_t]) if factor_t is not None else None
        h = C.c_void_p()
        capi.check(self._L.vm_video_create(self._ctx._h, n, ws, hs, ds, ft, int(depth0 if depth0 is not None else levels[0][2]), C.byref(h)))
        self._h = h
        self.levels = [tuple(int(x) for x in l) for l in levels]
        self.depth0 = int(depth0 if depth0 is not None else levels[0][2])
        self._vector = []
        self.factor_t = list(factor_t) if factor_t is not None else [1] + [2 if levels[i][2] != levels[i - 1][2] else 1 for i in range(1, n)]
        self.pages = [[VideoPage(self, l, t, levels[l][0], levels[l][1]) for t in range(levels[l][2])] for l in range(n)]

    def result(self, lvl, w0=None, h0=None):
        """CMatchingThread::update_result for depth > 1 (MatchingThread.cpp:22-84): the depth0
        full-resolution frames of the halfway field from level `lvl` -- every page scaled and
        resized, the frames the temporal pyramid skipped blended from their neighbours"""
        w0 = int(w0 if w0 is not None else self.levels[0][0])
        h0 = int(h0 if h0 is not None else self.levels[0][1])
        out = np.zeros((self.depth0, h0, w0, 2), dtype=np.float32)
        capi.check(self._L.vm_video_result(self._h, int(lvl), w0, h0, out.ctypes.data))
        return out

    def factor_d(self, lvl):
        f = C.c_float(0)
        capi.check(self._L.vm_video_level_dims(self._h, lvl, None, None, None, C.byref(f)))
        return f.value

    def upload_luma(self, lvl, page, img0, img1):
        img0 = np.ascontiguousarray(img0, dtype=np.float32)
        img1 = np.ascontiguousarray(img1, dtype=np.float32)
        capi.check(self._L.vm_video_upload_luma(self._h, lvl, page, img0.ctypes.data, img1.ctypes.data, 0))

    def upload_flows(self, lvl, page, f0, f1, b0, b1):
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in (f0, f1, b0, b1)]
        capi.check(self._L.vm_video_upload_flows(self._h, lvl, page, *[x.ctypes.data for x in a], 0))

    def build_flows(self, f0, f1, b0, b1):
        """flow half of Pyramid::build on the device from the full-resolution flows of every frame"""
        fam = [[np.ascontiguousarray(x, dtype=np.float32) for x in f] for f in (f0, f1, b0, b1)]
        n = len(fam[0])
        ptrs = [(C.c_void_p * n)(*[a.ctypes.data for a in f]) for f in fam]
        capi.check(self._L.vm_video_build_flows(self._h, *ptrs))

    def build_rgb_frame(self, frame, rgb0, rgb1):
        rgb0 = np.ascontiguousarray(rgb0, dtype=np.uint8)
        rgb1 = np.ascontiguousarray(rgb1, dtype=np.uint8)
        capi.check(self._L.vm_video_build_rgb(self._h, int(frame), rgb0.ctypes.data, rgb1.ctypes.data, 0))

    def build_flows_rgb(self, video0, video1, flow_params=None):
        """MdiEditor::OpticalFlow (UI/MdiEditor.cpp:1584-1689) of both RGB8 videos on the device, then the
        flow half of Pyramid::build; the flows never leave the device"""
        v = [[np.ascontiguousarray(x, dtype=np.uint8) for x in vid] for vid in (video0, video1)]
        n = len(v[0])
        ptrs = [(C.c_void_p * n)(*[a.ctypes.data for a in vid]) for vid in v]
        capi.check(self._L.vm_video_build_flows_rgb(self._h, ptrs[0], ptrs[1], 0, _flow_params(flow_params)))

    def build_rgb(self, video0, video1, start_res, flow_params=None):
        """OpticalFlow(); pyramid.build(v1, v2, f1, f2, b1, b2, start_res) (UI/MdiEditor.cpp:499-512) for RGB8
        videos (d, h, w, 3): the level table of synth.video_levels, the device image chain per frame
        (vm_video_build_rgb) and the flows computed on the device"""
        d, h, w = len(video0), video0[0].shape[0], video0[0].shape[1]
        levels, factor_t = synth.video_levels(w, h, d, start_res)
        self.build_levels(levels, factor_t, d)
        for t in range(d):
            self.build_rgb_frame(t, video0[t], video1[t])
        self.build_flows_rgb(video0, video1, flow_params)

    def build(self, video0, video1, f0, f1, b0, b1, start_res):
        """Pyramid::build(video0, video1, f0, f1, b0, b1, start_res), pyramid.cu:166-485, for float
        luma frames: geometry incl. the temporal pyramid (synth.video_levels), box-filtered lumas
        per page (as Pyramid.build of a pair does), flows through the device builder."""
        h, w = video0[0].shape
        d = len(video0)
        levels, factor_t = synth.video_levels(w, h, d, start_res)
        self.build_levels(levels, factor_t, d)
        frames = synth.page_frames(levels, factor_t)
        pyr = [synth.build_pyramid(video0[t], video1[t], len(levels)) for t in range(d)]
        for l in range(len(levels) - 1):
            for t in range(levels[l][2]):
                self.upload_luma(l, t, *pyr[frames[l][t]][l])
        self.build_flows(f0, f1, b0, b1)


class VideoMorph(object):
    """class Morph (morph.h:10-31) over a VideoPyramid: the temporally coupled solve."""

    def __init__(self, params, pyramid, run_flag=None, fixed_work=False):
        self.m_params, self.m_pyramid = params, pyramid
        self.m_cb = run_flag if run_flag is not None else C.c_int(1)
        self.fixed_work = bool(fixed_work)
        self._max_iter = float(params.max_iter)
        self.progress = {}
        self.energies = {}   # level -> [the five totals of every page] (VideoPage.energy()), filled when the solve returns

    def calculate_halfway_parametrization(self):
        """morph.cu:150-168 with the page schedule of optimize_level (:1353-1441)"""
        P, vid = self.m_params, self.m_pyramid
        vid._ctx.set_params(KernParameters(P))
        cons, n = _vcons_array(video_constraints(P))
        flag = C.cast(C.pointer(self.m_cb), C.c_void_p)
        total = sum(l[2] for l in vid.levels[:-1])
        prog = (capi.Progress * total)()
        capi.check(vid._L.vm_video_solve(vid._h, self._max_iter, float(P.max_iter_drop_factor), cons, n, flag,
                                         int(self.fixed_work), prog))
        k = 0
        for l in range(len(vid.levels) - 1):
            for t in range(vid.levels[l][2]):
                pr = prog[k]
                self.progress[(l, t)] = dict(iters=pr.iters, iters_live=pr.iters_live, improving=pr.improving, commits=pr.commits,
                                             candidates=pr.candidates, elapsed_ms=pr.elapsed_ms)
                k += 1
            # (the levels of one vm_video_solve are pipelined inside the call: the totals are read once it is back)
            self.energies[l] = [pg.energy() for pg in vid.pages[l]]
        return True


class VideoMatchingThread(_SolverThread):
    """class CMatchingThread (MatchingThread.h:7-37) over a video pair: the temporally coupled solve on
    a worker thread, then update_result() -- pyramid._vector[frame] for every frame of the video,
    at w0 x h0 (the size of the reference's placeholder level pyramid[0]; default: the finest level's)."""

    def __init__(self, parameters, pyramids, w0=None, h0=None, fixed_work=False):
        _SolverThread.__init__(self)
        self._parameters, self._pyramids = parameters, pyramids
        self.w0 = int(w0 if w0 is not None else pyramids.levels[0][0])
        self.h0 = int(h0 if h0 is not None else pyramids.levels[0][1])
        self.gpu_morph = VideoMorph(parameters, pyramids, self._flag, fixed_work)

    @property
    def energies(self):
        """{level: [the five energy totals of every page]} (VideoMorph.energies)"""
        return self.gpu_morph.energies

    def _solve(self):
        """MatchingThread.cpp:138-150"""
        self.gpu_morph.calculate_halfway_parametrization()

    def update_result(self, lvl=0):
        """MatchingThread.cpp:22-84 (the level the solver has reached; after run(): the finest)"""
        self._pyramids._vector = list(self._pyramids.result(lvl, self.w0, self.h0))
        self.percentage = 100.0


# ---- synchronisation stage: CSyncThread (SyncThread.h:7-39) + the stage-1 renderer ------------

def sync_constraints(P):
    """Resolve lp / rp / cnt the way CSyncThread::genMatrix walks them (SyncThread.cpp:155-165):
    every Connect ties (x, y, frame) of video 0 to (x, y, frame) of video 1."""
    out = []
    for row in P.cnt:
        for c in row:
            l, r = P.lp[c.li[0]][c.li[1]], P.rp[c.ri[0]][c.ri[1]]
            out.append((int(l.p[0]), int(l.p[1]), int(l.p[2]), int(r.p[0]), int(r.p[1]), int(r.p[2])))
    return out


def sync_level_table(w, h, d, start_res):
    """[(w, h, d)] of Pyramid::build(video0, video1, f0, f1, start_res): entry 0 = full resolution"""
    L = capi.load()
    lw, lh, ld = ((C.c_int * 64)() for _ in range(3))
    n = C.c_int(0)
    capi.check(L.vm_sync_level_table(int(w), int(h), int(d), int(start_res), lw, lh, ld, 64, C.byref(n)))
    return [(lw[i], lh[i], ld[i]) for i in range(n.value)]


class SyncPyramid(object):
    """What class Pyramid holds after build(video0, video1, f0, f1, start_res) (pyramid.cu:57-165):
    the level table, the four layered arrays the stage-1 renderer samples, and _vector."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, capi.load()
        self._h = None
        self.levels = []
        self._vector = []

    def clear(self):
        if getattr(self, "_h", None):
            self._L.vm_sync_destroy(self._h)
            self._h = None

    __del__ = clear

    def size(self):
        return len(self.levels)

    def build_levels(self, levels):
        self.clear()
        n = len(levels)
        ws = (C.c_int * n)(*[int(l[0]) for l in levels])
        hs = (C.c_int * n)(*[int(l[1]) for l in levels])
        ds = (C.c_int * n)(*[int(l[2]) for l in levels])
        h = C.c_void_p()
        capi.check(self._L.vm_sync_create(self._ctx._h, n, ws, hs, ds, C.byref(h)))
        self._h = h
        self.levels = [tuple(int(x) for x in l) for l in levels]
        w0, h0, d0 = self.levels[0]
        self._vector = [np.zeros((h0, w0, 4), np.float32) for _ in range(d0)]

    def build(self, video0, video1, f0, f1, start_res):
        """video*: (d, h, w, 3 or 4) u8; f*: (d, h, w, 2) float32 forward flows"""
        d, h, w = video0.shape[:3]
        self.build_levels(sync_level_table(w, h, d, start_res))
        for side, (vid, fl) in enumerate(((video0, f0), (video1, f1))):
            for t in range(d):
                self.upload_frame(side, t, vid[t])
                self.upload_flow(side, t, fl[t])

    def upload_frame(self, side, frame, rgb):
        rgb = np.asarray(rgb, np.uint8)
        if rgb.shape[-1] == 3:
            rgb = np.concatenate([rgb, np.zeros(rgb.shape[:2] + (1,), np.uint8)], axis=-1)
        rgb = np.ascontiguousarray(rgb)
        capi.check(self._L.vm_sync_upload_frame(self._h, side, frame, rgb.ctypes.data, rgb.shape[1] * 4))

    def compute_flows(self, params=None):
        """the forward flows of both uploaded videos (MdiEditor::OpticalFlow, UI/MdiEditor.cpp:1584-1689),
        computed on the device into the renderer's flow arrays"""
        capi.check(self._L.vm_sync_compute_flows(self._h, _flow_params(params)))

    def upload_flow(self, side, frame, flow):
        flow = np.ascontiguousarray(flow, np.float32)
        capi.check(self._L.vm_sync_upload_flow(self._h, side, frame, flow.ctypes.data, flow.shape[1] * 2))

    def field(self, lvl):
        """(X, Y, Z) of level lvl, each (d, h, w) float32"""
        w, h, d = self.levels[lvl]
        out = [np.zeros((d, h, w), np.float32) for _ in range(3)]
        capi.check(self._L.vm_sync_get_field(self._h, lvl, *[o.ctypes.data for o in out]))
        return out

    def set_field(self, lvl, X, Y, Z):
        a = [np.ascontiguousarray(t, np.float32) for t in (X, Y, Z)]
        capi.check(self._L.vm_sync_set_field(self._h, lvl, *[t.ctypes.data for t in a]))

    def result(self, lvl, frame):
        w0, h0, _ = self.levels[0]
        out = np.zeros((h0, w0, 4), np.float32)
        capi.check(self._L.vm_sync_result(self._h, lvl, frame, out.ctypes.data))
        return out

    def render_resample(self, fa, frame):
        """RenderWidget::RenderStage1 (UI/RenderWidget.cpp:205-227) -> (h, w, 3) u8"""
        w0, h0, _ = self.levels[0]
        out = np.zeros((h0, w0, 3), np.uint8)
        capi.check(self._L.vm_sync_render(self._h, float(fa), int(frame), out.ctypes.data, w0 * 3))
        return out

    def render_resample_dev(self, fa, frame):
        ms = C.c_float(0)
        capi.check(self._L.vm_sync_render_dev(self._h, float(fa), int(frame), C.byref(ms)))
        return ms.value


class SyncThread(_SolverThread):
    """class CSyncThread (SyncThread.h:7-39) on threading.Thread: runflag, percentage, run_time,
    run(), update_result()."""

    def __init__(self, parameters, pyramids):
        _SolverThread.__init__(self)
        self._parameters, self._pyramids = parameters, pyramids
        self._total_l = pyramids.size() - 1
        self._current_l = self._total_l
        self._max_iter = float(parameters.max_iter * 10)
        self._current_iter = 0.0
        self._total_iter = 0.0
        it = parameters.max_iter * 10
        for el in range(self._total_l, 0, -1):  # SyncThread.cpp:15-22 (integer division by the drop factor)
            w, h, d = pyramids.levels[el]
            self._total_iter += float(it) * w * h * d
            it = int(it / parameters.max_iter_drop_factor)
        self.progress = {}

    def load_identity(self, el):
        capi.check(self._pyramids._L.vm_sync_load_identity(self._pyramids._h, el))

    def upsample_level(self, el, pel=None):
        capi.check(self._pyramids._L.vm_sync_upsample_level(self._pyramids._h, el))

    def optimize_level(self, el):
        pyr = self._pyramids
        pyr._ctx.set_params(KernParameters(self._parameters))
        cons = sync_constraints(self._parameters)
        arr = (capi.SyncConstraint * max(len(cons), 1))()
        for i, c in enumerate(cons):
            arr[i] = capi.SyncConstraint(*c)
        capi.check(pyr._L.vm_sync_set_constraints(pyr._h, arr, len(cons)))
        pr = capi.SyncProgress()
        capi.check(pyr._L.vm_sync_optimize_level(pyr._h, el, self._max_iter, self._flag_ptr(), C.byref(pr)))
        self.progress[el] = dict(iters=pr.iters, launches=pr.launches, voxel_iters=pr.voxel_iters,
                                 elapsed_ms=pr.elapsed_ms, resid=tuple(pr.resid))
        self._current_iter += pr.voxel_iters
        return pr

    def _solve(self):
        """SyncThread.cpp:58-84"""
        self._current_l = self._total_l
        while self._current_l > 0:
            el = self._current_l
            if el == self._total_l:
                self.load_identity(el)
            else:
                self.upsample_level(el, el + 1)
            self.optimize_level(el)
            self._max_iter = float(np.float32(self._max_iter) / np.float32(2))
            if not self.runflag:
                break
            self._current_l -= 1

    def update_result(self):
        """SyncThread.cpp:482-521: _vector[z] = (X ratio_x, Y ratio_y, Z, 0) resized to full size"""
        pyr = self._pyramids
        el = max(self._current_l, 1)
        for z in range(pyr.levels[el][2]):
            pyr._vector[z] = pyr.result(el, z)
        self.percentage = (self._current_iter / self._total_iter * 100.0) if self._total_iter else 100.0


# ---- dense optical flow (MdiEditor::OpticalFlow, UI/MdiEditor.cpp:1584-1689) ---------------------------

class FlowParams(capi.FlowParams):
    """cuda::FarnebackOpticalFlow's settings; FlowParams() holds the reference's defaults, keywords override"""

    def __init__(self, **kw):
        capi.FlowParams.__init__(self)
        capi.check(capi.load().vm_flow_params_default(C.byref(self)))
        for k, v in kw.items():
            if k not in dict(capi.FlowParams._fields_):
                raise TypeError("FlowParams has no field %r" % k)
            setattr(self, k, v)


def _flow_params(params):
    return None if params is None else C.byref(params)


def optical_flow(ctx, frames_a, frames_b, params=None):
    """n flows a[i] -> b[i] (b(x + d) ~ a(x)) in the same launches: frames (n, h, w, 3) uint8 or
    (n, h, w) float luma (a single frame without the leading n is accepted); returns (n, h, w, 2) float32"""
    a, b = np.asarray(frames_a), np.asarray(frames_b)
    rgb = a.dtype == np.uint8
    if a.ndim == (3 if rgb else 2):
        a, b = a[None], b[None]
    if a.shape != b.shape or a.ndim != (4 if rgb else 3) or (rgb and a.shape[-1] != 3):
        raise ValueError("optical_flow: frames of shape %s and %s" % (a.shape, b.shape))
    a = np.ascontiguousarray(a, np.uint8 if rgb else np.float32)
    b = np.ascontiguousarray(b, np.uint8 if rgb else np.float32)
    n, h, w = a.shape[:3]
    out = np.zeros((n, h, w, 2), np.float32)
    pa = (C.c_void_p * n)(*[a[i].ctypes.data for i in range(n)])
    pb = (C.c_void_p * n)(*[b[i].ctypes.data for i in range(n)])
    po = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
    fn = ctx._L.vm_optical_flow_rgb if rgb else ctx._L.vm_optical_flow_luma
    capi.check(fn(ctx._h, w, h, n, pa, pb, 0, _flow_params(params), po))
    return out


def video_optical_flows(ctx, video0, video1, params=None):
    """MdiEditor::OpticalFlow of two videos (d frames each, RGB8 or float luma): (f0, f1, b0, b1), each
    (d, h, w, 2); f[t] = t -> t + 1 (zero for the last frame), b[t] = t -> t - 1 (zero for frame 0).  All
    4 (d - 1) flows go through one vm_optical_flow_* call as independent pairs (a frame is expanded once per
    pair it is in; VideoPyramid.build_rgb keeps the flows on the device and expands each frame once)."""
    v0, v1 = np.asarray(video0), np.asarray(video1)
    d = len(v0)
    out = [np.zeros(v0.shape[:3] + (2,), np.float32) for _ in range(4)]
    if d < 2:
        return tuple(out)
    a = np.concatenate([v0[:-1], v1[:-1], v0[1:], v1[1:]])
    b = np.concatenate([v0[1:], v1[1:], v0[:-1], v1[:-1]])
    fl = optical_flow(ctx, a, b, params)
    m = d - 1
    out[0][:-1], out[1][:-1], out[2][1:], out[3][1:] = fl[:m], fl[m:2 * m], fl[2 * m:3 * m], fl[3 * m:]
    return tuple(out)


# ---- key-point tracks of stage 2 (MdiEditor::AddPoint / MovePoint / NextStage, UI/MdiEditor.cpp) -------

TRACK_POINT = np.dtype([("x", "<i4"), ("y", "<i4"), ("weight", "<f4")])


class PointTracker(object):
    """MdiEditor's resample1/2, f1/f2, b1/b2 on the device (vm_track): the full-resolution RGB8 frames
    of both videos (d, h, w, 3) and their flows.  flows = (f0, f1, b0, b1), each (d, h, w, 2) as
    video_optical_flows returns them; None: computed on the device (vm_track_compute_flows)."""

    def __init__(self, ctx, video0, video1, flows=None, flow_params=None):
        self._ctx, self._L = ctx, capi.load()
        self._h = None
        v = [np.asarray(x) for x in (video0, video1)]
        if v[0].shape != v[1].shape or v[0].ndim != 4 or v[0].shape[-1] != 3 or v[0].dtype != np.uint8:
            raise ValueError("PointTracker: two RGB8 videos (d, h, w, 3) of one shape wanted")
        self.depth, self.height, self.width = v[0].shape[:3]
        h = C.c_void_p()
        capi.check(self._L.vm_track_create(ctx._h, self.width, self.height, self.depth, C.byref(h)))
        self._h = h
        for side in range(2):
            for t in range(self.depth):
                fr = np.ascontiguousarray(v[side][t])
                capi.check(self._L.vm_track_upload_frame(self._h, side, t, fr.ctypes.data, 0))
        if flows is None:
            capi.check(self._L.vm_track_compute_flows(self._h, _flow_params(flow_params)))
        else:
            fam = [np.ascontiguousarray(x, dtype=np.float32) for x in flows]
            for side in range(2):
                for t in range(self.depth):
                    capi.check(self._L.vm_track_upload_flows(self._h, side, t, fam[side][t].ctypes.data,
                                                             fam[2 + side][t].ctypes.data, 0))

    def close(self):
        if getattr(self, "_h", None):
            self._L.vm_track_destroy(self._h)
            self._h = None

    __del__ = close

    def get_flows(self, side, frame):
        """(f[frame], b[frame]) of video `side`, each (h, w, 2) float32"""
        f = np.zeros((self.height, self.width, 2), np.float32)
        b = np.zeros_like(f)
        capi.check(self._L.vm_track_get_flows(self._h, int(side), int(frame), f.ctypes.data, b.ctypes.data))
        return f, b

    def propagate(self, segments):
        """vm_track_propagate: segments [(side, x, y, frame, ox, oy, ofr, dir)] -> (n, depth) TRACK_POINT array;
        only the frames a segment covers are written (the rest stay zero)"""
        n = len(segments)
        segs = (capi.TrackSegment * max(n, 1))()
        for i, s in enumerate(segments):
            segs[i] = capi.TrackSegment(*[int(v) for v in s])
        out = np.zeros((n, self.depth), TRACK_POINT)
        capi.check(self._L.vm_track_propagate(self._h, segs, n, out.ctypes.data))
        return out


def _segment_tuple(side, seg):
    """("chain", key, dir) / ("blend", m, o) with keys (x, y, z) -> the vm_track_segment fields"""
    if seg[0] == "chain":
        k = seg[1]
        return (side, k[0], k[1], k[2], 0, 0, -1, seg[2])
    m, o = seg[1], seg[2]
    return (side, m[0], m[1], m[2], o[0], o[1], o[2], 0)


def _covered(seg, d):
    if seg[0] == "chain":
        z = seg[1][2]
        return range(z + 1, d) if seg[2] > 0 else range(0, z)
    a, b = sorted((seg[1][2], seg[2][2]))
    return range(a + 1, b)


def _apply(track, seg, row, d):
    for s in _covered(seg, d):
        track[s] = Conp(int(row[s]["x"]), int(row[s]["y"]), s, 0, float(row[s]["weight"]))


def _track_points(P, side):
    return P.lp if side == 0 else P.rp


def _add_point(self, side, x, y, frame, tracker):
    """MdiEditor::AddPoint (UI/MdiEditor.cpp:1230-1276) on the device: a new track of `side` (0 = lp, 1 = rp)
    from the key (x, y) at `frame`, walked through every other frame; returns the track's index"""
    d = tracker.depth
    key = (int(x), int(y), int(frame))
    segs = [("chain", key, -1), ("chain", key, 1)]
    out = tracker.propagate([_segment_tuple(side, s) for s in segs])
    track = [None] * d
    track[key[2]] = Conp(key[0], key[1], key[2], 1, 1.0)
    for s, row in zip(segs, out):
        _apply(track, s, row, d)
    pts = _track_points(self, side)
    pts.append(track)
    return len(pts) - 1


def _move_point(self, side, track, frame, x, y, tracker):
    """MdiEditor::MovePoint (UI/MdiEditor.cpp:1279-1393) on the device: the key of `track` at `frame` becomes
    (x, y); the frames up to the neighbouring keys (or the ends) are propagated again, blended with the
    neighbours' chains"""
    pts = _track_points(self, side)[track]
    d = len(pts)
    frame = int(frame)
    pts[frame] = Conp(int(x), int(y), frame, 1, 1.0)
    m = (int(x), int(y), frame)
    beg = next((j for j in range(frame - 1, -1, -1) if pts[j].p[3]), None)
    end = next((j for j in range(frame + 1, d) if pts[j].p[3]), None)
    segs = [("chain", m, -1) if beg is None else ("blend", m, pts[beg].p[:3]),
            ("chain", m, 1) if end is None else ("blend", m, pts[end].p[:3])]
    out = tracker.propagate([_segment_tuple(side, s) for s in segs])
    for s, row in zip(segs, out):
        _apply(pts, s, row, d)


def _connect_point(self, l_track, r_track):
    """the stage-2 branch of MdiEditor::ConnectPoint (UI/MdiEditor.cpp:1395-1475, thread_flag >= 2): a per-frame
    list (l_track, t) - (r_track, t) is added when neither track is connected, removed when exactly this pair
    is; nothing happens when only one of them is connected elsewhere"""
    for k, row in enumerate(self.cnt):
        for c in row:
            if c.li[0] == l_track or c.ri[0] == r_track:
                if c.li[0] == l_track and c.ri[0] == r_track:
                    del self.cnt[k]
                return
    d = len(self.lp[l_track])
    self.cnt.append([Connect((l_track, t), (r_track, t)) for t in range(d)])


Parameters.add_point = _add_point
Parameters.move_point = _move_point
Parameters.connect_point = _connect_point


def stage_two_parameters(P_sync, tracker):
    """NextStage's points section (UI/MdiEditor.cpp:1714-1791): stage-1 connection j of list i becomes a key at
    ((x, y), (lz + rz) / 2) on track i of either side -- AddPoint for j = 0, MovePoint for a later j -- and list
    i becomes the d connects (i, t) - (i, t).  All segments of both sides go through ONE vm_track_propagate
    call, in the segment form.  Returns a new Parameters with P_sync's settings.  An empty
    stage-1 list (which the editor never leaves) is a ValueError."""
    import copy
    P = copy.copy(P_sync)
    P.lp, P.rp, P.cnt = [], [], []
    d = tracker.depth
    keys = [[], []]  # per side, per list: {z: ((x, y, z), time of the last edit)}
    for i, row in enumerate(P_sync.cnt):
        if not row:
            raise ValueError("stage_two_parameters: stage-1 connection list %d is empty" % i)
        kk = [{}, {}]
        for j, c in enumerate(row):
            l, r = P_sync.lp[c.li[0]][c.li[1]].p, P_sync.rp[c.ri[0]][c.ri[1]].p
            z = int((l[2] + r[2]) // 2 + 0.5)
            kk[0][z] = ((l[0], l[1], z), j)
            kk[1][z] = ((r[0], r[1], z), j)
        keys[0].append(kk[0])
        keys[1].append(kk[1])
    jobs = []  # (side, list, segment)
    for side in range(2):
        for i, kk in enumerate(keys[side]):
            zs = sorted(kk)
            jobs.append((side, i, ("chain", kk[zs[0]][0], -1)))
            jobs.append((side, i, ("chain", kk[zs[-1]][0], 1)))
            for a, b in zip(zs, zs[1:]):
                (ka, ta), (kb, tb) = kk[a], kk[b]
                jobs.append((side, i, ("blend", ka, kb) if ta > tb else ("blend", kb, ka)))
    out = tracker.propagate([_segment_tuple(side, s) for side, _, s in jobs])
    tracks = [[[None] * d for _ in keys[0]], [[None] * d for _ in keys[1]]]
    for side in range(2):
        for i, kk in enumerate(keys[side]):
            for z, (k, _) in kk.items():
                tracks[side][i][z] = Conp(k[0], k[1], z, 1, 1.0)
    for (side, i, s), row in zip(jobs, out):
        _apply(tracks[side][i], s, row, d)
    P.lp, P.rp = tracks
    P.cnt = [[Connect((i, t), (i, t)) for t in range(d)] for i in range(len(keys[0]))]
    return P


def _video_build_flows_track(self, tracker):
    """the flow half of Pyramid::build from the tracker's flows (device to device): NextStage's one
    OpticalFlow serves the tracks and the stage-2 pyramid"""
    capi.check(self._L.vm_video_build_flows_track(self._h, tracker._h))


VideoPyramid.build_flows_track = _video_build_flows_track
