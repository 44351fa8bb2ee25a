"""ctypes binding of the CPU oracle (oracle/vm_oracle.h).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg.  The product package never imports this.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_ODIR = os.path.join(_ROOT, "oracle")
# VM_ORACLE_SO: an alternative build of the oracle (e.g. with -fsanitize=address,undefined)
_SO = os.environ.get("VM_ORACLE_SO") or os.path.join(_ODIR, "_build", "libvm_oracle.so")


def build(force=False):
    srcs = [os.path.join(_ODIR, f) for f in os.listdir(_ODIR) if f.endswith((".c", ".h"))]
    stale = (not os.path.exists(_SO)) or any(
        os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs)
    if "VM_ORACLE_SO" in os.environ:
        return _SO
    if force or stale:
        subprocess.check_call(["make", "-C", _ODIR], stdout=subprocess.DEVNULL)
    return _SO


class Params(C.Structure):
    _fields_ = [("w_temp", C.c_float), ("w_ui", C.c_float), ("w_tps", C.c_float),
                ("w_ssim", C.c_float), ("ssim_clamp", C.c_float), ("eps", C.c_float),
                ("bcond", C.c_int)]


class Constraint(C.Structure):
    _fields_ = [("lx", C.c_float), ("ly", C.c_float), ("rx", C.c_float),
                ("ry", C.c_float), ("weight", C.c_float)]


def default_params(**kw):
    """Reference defaults, UI/MdiEditor.cpp:131-140."""
    p = Params(w_temp=10.0, w_ui=1e5, w_tps=0.05, w_ssim=100.0, ssim_clamp=0.0,
               eps=0.01, bcond=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def make_constraints(arr):
    arr = np.asarray(arr, dtype=np.float32).reshape(-1, 5)
    cs = (Constraint * max(len(arr), 1))()
    for i, r in enumerate(arr):
        cs[i] = Constraint(*[float(x) for x in r])
    return cs, len(arr)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(build())
    L.vmo_calc_border.restype = C.c_int
    L.vmo_calc_border.argtypes = [C.c_int, C.c_int]
    L.vmo_ssim.restype = C.c_float
    L.vmo_ssim.argtypes = [C.c_float] * 7
    L.vmo_tex2d.restype = C.c_float
    L.vmo_tex2d.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
    for f in ("vmo_tps_stencil", "vmo_tps_rows_from_dense", "vmo_io_stencil",
              "vmo_improvmask_stencil"):
        getattr(L, f).argtypes = [C.c_void_p]
        getattr(L, f).restype = None
    L.vmo_level_create.restype = C.c_void_p
    L.vmo_level_create.argtypes = [C.c_int, C.c_int]
    L.vmo_level_destroy.argtypes = [C.c_void_p]
    L.vmo_level_destroy.restype = None
    L.vmo_level_field.restype = C.c_void_p
    L.vmo_level_field.argtypes = [C.c_void_p, C.c_int]
    L.vmo_init_level.argtypes = [C.c_void_p, C.c_float]
    L.vmo_init_level.restype = None
    L.vmo_splat_constraints.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.vmo_splat_constraints.restype = None
    L.vmo_optimize_iter.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p]
    L.vmo_optimize_iter.restype = C.c_int
    L.vmo_optimize_level.argtypes = [C.c_void_p, C.POINTER(Params), C.c_float, C.c_void_p]
    L.vmo_optimize_level.restype = C.c_int
    L.vmo_upsample_v.argtypes = [C.c_void_p, C.c_void_p]
    L.vmo_upsample_v.restype = None
    L.vmo_coarse_solve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params),
                                   C.c_void_p, C.c_int]
    L.vmo_coarse_solve.restype = C.c_int
    L.vmo_coarse_solve_page.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params),
                                        C.c_void_p, C.c_int, C.c_int]
    L.vmo_coarse_solve_page.restype = C.c_int
    L.vmo_energy.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p]
    L.vmo_energy.restype = None
    L.vmo_render_halfway.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                     C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    L.vmo_render_halfway.restype = None
    L.vmo_upscale_result.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.vmo_upscale_result.restype = None
    L.vmo_blend_v.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_size_t]
    L.vmo_blend_v.restype = None
    L.vmo_poisson_extend.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p]
    L.vmo_poisson_extend.restype = C.c_int
    L.vmo_poisson_prepare.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p]
    L.vmo_poisson_prepare.restype = C.c_int
    L.vmo_dbg_foldover.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_float, C.c_float]
    L.vmo_dbg_foldover.restype = C.c_float
    L.vmo_dbg_energy_change.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_float, C.c_float]
    L.vmo_dbg_energy_change.restype = C.c_float
    L.vmo_quadratic_path.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_double)]
    L.vmo_quadratic_path.restype = C.c_int
    L.vmo_luma_pyramid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.vmo_luma_pyramid.restype = None
    L.vmo_scale_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.vmo_scale_planes.restype = None
    L.vmo_level_set_temporal.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.vmo_level_set_temporal.restype = None
    L.vmo_temp_splat.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vmo_temp_splat.restype = None
    L.vmo_temp_normalise.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vmo_temp_normalise.restype = None
    L.vmo_initialize_temp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vmo_initialize_temp.restype = None
    L.vmo_temporal_fill.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7
    L.vmo_temporal_fill.restype = None
    L.vmo_flow_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.vmo_flow_scale.restype = None
    L.vmo_flow_concat.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.vmo_flow_concat.restype = None
    L.vmo_set_commit_order.argtypes = [C.c_int]
    L.vmo_set_commit_order.restype = None
    L.vmo_set_tex_filter.argtypes = [C.c_int]
    L.vmo_set_tex_filter.restype = None
    L.vmo_get_tex_filter.restype = C.c_int
    L.vmo_set_threads.argtypes = [C.c_int]
    L.vmo_set_threads.restype = None
    L.vmo_get_threads.restype = C.c_int
    L.vmo_sync_levels.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int]
    L.vmo_sync_levels.restype = C.c_int
    L.vmo_sync_row.argtypes = [C.c_int] * 6 + [C.c_float, C.c_float, C.c_void_p]
    L.vmo_sync_row.restype = None
    L.vmo_sync_state.argtypes = [C.c_int, C.c_int]
    L.vmo_sync_state.restype = C.c_int
    L.vmo_sync_table.argtypes = [C.c_int] * 3 + [C.c_float, C.c_void_p]
    L.vmo_sync_table.restype = None
    L.vmo_sync_ui.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 4
    L.vmo_sync_ui.restype = None
    L.vmo_sync_diag.argtypes = [C.c_int] * 3 + [C.c_float, C.c_void_p, C.c_void_p]
    L.vmo_sync_diag.restype = None
    L.vmo_sync_dot.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 3
    L.vmo_sync_dot.restype = C.c_float
    L.vmo_sync_apply.argtypes = [C.c_int] * 3 + [C.c_float] + [C.c_void_p] * 3
    L.vmo_sync_apply.restype = None
    L.vmo_sync_solve_level.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float] + [C.c_void_p] * 4
    L.vmo_sync_solve_level.restype = C.c_int
    L.vmo_sync_upsample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float]
    L.vmo_sync_upsample.restype = None
    L.vmo_sync_result.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]
    L.vmo_sync_result.restype = None
    L.vmo_render_resample.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_float, C.c_int] + [C.c_void_p] * 5
    L.vmo_render_resample.restype = None
    L.vmo_set_threads(default_threads())
    _lib = L
    return L


def default_threads():
    """OpenMP threads for the oracle: the CPUs this process may really use (affinity mask capped
    by the cgroup quota -- a 256-thread team on a 16-CPU quota is ~100x slower), at most 8"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(q) // int(per)))
    except Exception:
        pass
    return max(1, min(n, 8))


_FIELDS = {  # name -> (id, channels, dtype)
    "img0": (0, 1, np.float32), "img1": (1, 1, np.float32), "v": (2, 2, np.float32),
    "luma": (3, 2, np.float32), "mean": (4, 2, np.float32), "var": (5, 2, np.float32),
    "cross": (6, 1, np.float32), "value": (7, 1, np.float32), "counter": (8, 1, np.float32),
    "tps_axy": (9, 1, np.float32), "tps_b": (10, 2, np.float32),
    "ui_axy": (11, 1, np.float32), "ui_b": (12, 2, np.float32),
    "temp_ref": (14, 2, np.float32), "temp_mask": (15, 1, np.float32),
}


class Level:
    """One page of one pyramid level in the oracle (tight rows)."""

    def __init__(self, w, h):
        self.w, self.h = int(w), int(h)
        self.imp_rs = (self.w + 4) // 5 + 2
        self.imp_rows = (self.h + 4) // 5 + 2
        self._p = lib().vmo_level_create(self.w, self.h)

    def __del__(self):
        try:
            if self._p:
                lib().vmo_level_destroy(self._p)
                self._p = None
        except Exception:
            pass

    def field(self, name):
        """numpy VIEW of a field (h,w) or (h,w,2)."""
        if name == "impmask":
            ptr = lib().vmo_level_field(self._p, 13)
            n = self.imp_rs * self.imp_rows
            buf = (C.c_uint32 * n).from_address(ptr)
            return np.frombuffer(buf, dtype=np.uint32).reshape(self.imp_rows, self.imp_rs)
        fid, ch, dt = _FIELDS[name]
        ptr = lib().vmo_level_field(self._p, fid)
        n = self.w * self.h * ch
        buf = (C.c_float * n).from_address(ptr)
        a = np.frombuffer(buf, dtype=dt)
        return a.reshape(self.h, self.w, 2) if ch == 2 else a.reshape(self.h, self.w)

    def set_images(self, img0, img1):
        self.field("img0")[...] = img0
        self.field("img1")[...] = img1

    def init(self, ssim_clamp=0.0):
        lib().vmo_init_level(self._p, ssim_clamp)

    def splat(self, w0, h0, cons):
        cs, n = make_constraints(cons)
        lib().vmo_splat_constraints(self._p, w0, h0, cs, n)

    def optimize_iter(self, params, stats=None):
        sp = stats.ctypes.data if stats is not None else None
        return lib().vmo_optimize_iter(self._p, C.byref(params), sp)

    def optimize(self, params, max_iter, stats=None):
        sp = stats.ctypes.data if stats is not None else None
        return lib().vmo_optimize_level(self._p, C.byref(params), float(max_iter), sp)

    def upsample_from(self, src):
        lib().vmo_upsample_v(self._p, src._p)

    def coarse_solve(self, w0, h0, params, cons=(), depth=1):
        cs, n = make_constraints(cons)
        return lib().vmo_coarse_solve_page(self._p, w0, h0, C.byref(params), cs, n, int(depth))

    def set_temporal(self, flag, factor_d=1.0):
        lib().vmo_level_set_temporal(self._p, int(flag), float(factor_d))

    def initialize_temp(self, src, fa, fb):
        """initialize_temp(lvl, i, dir), upsample.cu:214-258: this page's temp.ref / temp.mask from
        the neighbouring page `src` advected by ITS flows (f0, f1 for dir < 0; b0, b1 for dir > 0)"""
        fa = np.ascontiguousarray(fa, dtype=np.float32)
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        lib().vmo_initialize_temp(self._p, src._p, fa.ctypes.data, fb.ctypes.data)

    def energy(self, params):
        out = np.zeros(3, dtype=np.float64)
        lib().vmo_energy(self._p, C.byref(params), out.ctypes.data)
        return out


def level_sizes(w, h, nlevels):
    """Level geometry rule of pyramid.cu:466-467 (ceil halving), integer math."""
    out = [(w, h)]
    for _ in range(nlevels - 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def solve(pyr_imgs, params, max_iter, drop=1.0, cons=(), stats=None, threads=None,
          per_level=None):
    """Morph::calculate_halfway_parametrization, morph.cu:150-168, on the oracle.

    pyr_imgs: list finest->coarsest of (img0, img1) float32 arrays; the last
    entry is the coarsest level (its images are not used: dense solve only).
    Returns the finest-level Level.
    """
    if threads:
        lib().vmo_set_threads(threads)
    h0, w0 = pyr_imgs[0][0].shape
    sizes = [im[0].shape[::-1] for im in pyr_imgs]
    cur = Level(*sizes[-1])
    cur.coarse_solve(w0, h0, params, cons)
    mi = float(max_iter)
    for el in range(len(pyr_imgs) - 2, -1, -1):
        lvl = Level(*sizes[el])
        lvl.set_images(*pyr_imgs[el])
        lvl.upsample_from(cur)
        lvl.init(params.ssim_clamp)
        lvl.splat(w0, h0, cons)
        it = lvl.optimize(params, mi, stats)
        if per_level is not None:
            per_level.append((sizes[el], it))
        mi = mi / drop
        cur = lvl
    return cur


def render_halfway(w, h, ex, color_fa, geo_fa, color_from, ext0, ext1, v, u):
    out = np.zeros((h, w, 3), dtype=np.uint8)
    ext0 = np.ascontiguousarray(ext0, dtype=np.float32)
    ext1 = np.ascontiguousarray(ext1, dtype=np.float32)
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = np.ascontiguousarray(u, dtype=np.float32)
    lib().vmo_render_halfway(out.ctypes.data, w, h, ex, color_fa, geo_fa, color_from,
                             ext0.ctypes.data, ext1.ctypes.data, v.ctypes.data, u.ctypes.data)
    return out


def upscale_result(v, w0, h0):
    v = np.ascontiguousarray(v, dtype=np.float32)
    h, w = v.shape[:2]
    out = np.zeros((h0, w0, 2), dtype=np.float32)
    lib().vmo_upscale_result(out.ctypes.data, w0, h0, v.ctypes.data, w, h)
    return out


def poisson_extend(ext_rgba, w, h, ex, other_rgba, v, side, tol=1e-8, max_it=20000):
    ext = np.ascontiguousarray(ext_rgba, dtype=np.uint8).copy()
    other = np.ascontiguousarray(other_rgba, dtype=np.uint8)
    v = np.ascontiguousarray(v, dtype=np.float32)
    rr = C.c_double(0)
    it = lib().vmo_poisson_extend(ext.ctypes.data, w, h, ex, other.ctypes.data,
                                  v.ctypes.data, side, tol, max_it, C.byref(rr))
    return ext, it, rr.value


def quadratic_path(v, tol=1e-10, max_it=200000, want_jopt=False):
    """CQuadraticPath::optimize for one frame: (u, iterations, residual[, j_opt])"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    h, w = v.shape[:2]
    u = np.zeros((h, w, 2), dtype=np.float32)
    jo = np.zeros((h, w, 4), dtype=np.float32)
    rr = C.c_double(0)
    it = lib().vmo_quadratic_path(v.ctypes.data, w, h, tol, max_it, u.ctypes.data, jo.ctypes.data, C.byref(rr))
    return (u, it, rr.value, jo) if want_jopt else (u, it, rr.value)


def poisson_prepare(ext_rgba, w, h, ex, other_rgba, v, side):
    ext = np.ascontiguousarray(ext_rgba, dtype=np.uint8).copy()
    other = np.ascontiguousarray(other_rgba, dtype=np.uint8)
    v = np.ascontiguousarray(v, dtype=np.float32)
    typ = np.zeros(((h + 2 * ex), (w + 2 * ex)), dtype=np.int32)
    n = lib().vmo_poisson_prepare(ext.ctypes.data, w, h, ex, other.ctypes.data,
                                  v.ctypes.data, side, typ.ctypes.data)
    return ext, typ, n


def luma_pyramid(rgb, nlevels):
    """list of level lumas (finest first) of the reference's Pyramid::build chain"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    sizes = level_sizes(w, h, nlevels)
    out = np.zeros(sum(a * b for a, b in sizes), dtype=np.float32)
    lib().vmo_luma_pyramid(rgb.ctypes.data, w, h, nlevels, out.ctypes.data)
    res, off = [], 0
    for (a, b) in sizes:
        res.append(out[off:off + a * b].reshape(b, a))
        off += a * b
    return res


def scale_planes(planes, wout, hout):
    """scale() of the pyramid chain alone: (3, h, w) float32 planes -> (3, hout, wout)"""
    planes = np.ascontiguousarray(planes, dtype=np.float32)
    _, h, w = planes.shape
    out = np.zeros((3, hout, wout), dtype=np.float32)
    lib().vmo_scale_planes(planes.ctypes.data, w, h, wout, hout, out.ctypes.data)
    return out


# ---------------------------------------------------------------------------------------------
# temporal coherence path: host control flow of the reference over the C kernels of
# oracle/vm_oracle_temporal.c


def video_geometry(w, h, d, start_res, max_stage2=14e6):
    """Level table of Pyramid::build (stage 2), pyramid.cu:223-240, 462-477, as the reference
    computes it: returns (levels, factor_t) with levels = [(w, h, d), ...] finest first incl. the
    coarsest (host-solved) level, factor_t[l] = temporal stride level l was built with.
    float32 logs and truncation, literally (the product side uses integer arithmetic,
    videomorphing_amd.synth.video_levels; tests compare the two)."""
    f32 = np.float32
    fa = max(np.sqrt(f32(w * h * d) / f32(max_stage2)), f32(1))
    w, h = int(w / fa), int(h / fa)
    lg = lambda v: np.log(f32(v)) / np.log(f32(2.0))      # pyramid.cu:51-56
    el_t = int(lg(d) - lg(start_res) + 1)
    el_y = int(lg(h) - lg(start_res) + 1)
    el_x = int(lg(w) - lg(start_res) + 1)
    el_x = el_y = max(el_x, el_y)
    maxl = max(el_x, el_t)
    levels, factors, factor_t = [], [], 1
    for el in range(maxl):
        levels.append((w, h, d))
        factors.append(factor_t)
        if maxl - el <= el_x:
            w = int(np.ceil(w / 2.0))
        if maxl - el <= el_y:
            h = int(np.ceil(h / 2.0))
        if maxl - el <= el_t:
            d, factor_t = int(np.ceil((d + 1) / 2.0)), 2
        else:
            factor_t = 1
    return levels, factors


def factor_d_table(depth0, depths):
    """pyramid.cu:470-477 over [placeholder level 0 (depth0)] + levels: factor_d per entry"""
    ds = [depth0] + list(depths)
    fd = [1.0] * len(ds)
    for i in range(len(ds) - 2, -1, -1):
        fd[i] = fd[i + 1] * 2 if ds[i + 1] != ds[i] else fd[i + 1]
    return fd


def flow_scale(flow, wout, hout):
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    h, w = flow.shape[:2]
    out = np.zeros((hout, wout, 2), dtype=np.float32)
    lib().vmo_flow_scale(flow.ctypes.data, w, h, wout, hout, out.ctypes.data)
    return out


def flow_concat(f, f_next):
    f = np.ascontiguousarray(f, dtype=np.float32).copy()
    f_next = np.ascontiguousarray(f_next, dtype=np.float32)
    h, w = f.shape[:2]
    lib().vmo_flow_concat(f.ctypes.data, f_next.ctypes.data, w, h)
    return f


def flow_pyramids(f0, f1, b0, b1, levels, factors):
    """All four flow families through Pyramid::build's loop.  f0.. : lists (one per frame) of
    full-resolution (h, w, 2) flows.  Returns per level (all but the coarsest, which holds no
    flows... the reference uploads flows for el < maxl-1 only) a dict name -> list of pages."""
    fam = {"f0": [np.asarray(x, np.float32) for x in f0], "f1": [np.asarray(x, np.float32) for x in f1],
           "b0": [np.asarray(x, np.float32) for x in b0], "b1": [np.asarray(x, np.float32) for x in b1]}
    out = []
    prev_d = levels[0][2]
    for el, (w, h, d) in enumerate(levels[:-1]):
        factor_t = factors[el]
        # every frame of the previous level to this level's size (el == 0: same size)
        for k in fam:
            fam[k] = [flow_scale(fl, w, h) for fl in fam[k][:prev_d]]
        if el > 0 and factor_t > 1:
            for t in range(d):
                if t * factor_t > prev_d - 1:
                    continue
                if t * factor_t + 1 < prev_d:
                    for k in ("f0", "f1"):
                        fam[k][t * factor_t] = flow_concat(fam[k][t * factor_t], fam[k][t * factor_t + 1])
                if t > 0:
                    for k in ("b0", "b1"):
                        fam[k][t * factor_t] = flow_concat(fam[k][t * factor_t], fam[k][t * factor_t - 1])
        if el > 0 and factor_t > 1:
            for k in fam:
                fam[k] = [fam[k][min(t * factor_t, prev_d - 1)].copy() for t in range(d)]
        out.append({k: [a.copy() for a in fam[k][:d]] for k in fam})
        prev_d = d
    return out


class Video:
    """A stage-2 pyramid of a video pair in the oracle: per level `d` pages (Level objects) and
    the four flow fields per page; the host side of Morph (morph.cu:150-168, 264-390,
    1353-1441) and of upsample() (upsample.cu:260-340) over it."""

    def __init__(self, levels, depth0=None):
        self.levels = [tuple(int(x) for x in l) for l in levels]
        self.depth0 = int(depth0 if depth0 is not None else self.levels[0][2])
        self.w0, self.h0 = self.levels[0][0], self.levels[0][1]
        self.factor_d = factor_d_table(self.depth0, [l[2] for l in self.levels])   # [0] = placeholder level
        self.pages = [[Level(w, h) for _ in range(d)] for (w, h, d) in self.levels]
        self.flows = [None] * len(self.levels)
        self.iters = {}

    def set_images(self, lvl, page, img0, img1):
        self.pages[lvl][page].set_images(img0, img1)

    def set_flows(self, lvl, fl):
        """fl: dict f0/f1/b0/b1 -> list of (h, w, 2) arrays, one per page"""
        self.flows[lvl] = {k: [np.ascontiguousarray(a, dtype=np.float32) for a in fl[k]] for k in fl}

    def _cons_for(self, lvl, z, cons):
        """constraints of page z of level lvl (morph.cu:351-358): rows (lx, ly, rx, ry, weight, frame)"""
        factor = int(self.factor_d[0] / self.factor_d[lvl + 1])
        conz = min(z * factor, self.depth0 - 1)
        cons = np.asarray(cons, dtype=np.float32).reshape(-1, 6)
        return cons[cons[:, 5] == conz][:, :5]

    def coarse_solve(self, P, cons=()):
        L = len(self.levels) - 1
        for z, pg in enumerate(self.pages[L]):
            pg.coarse_solve(self.w0, self.h0, P, self._cons_for(L, z, cons), depth=self.levels[L][2])

    def upsample(self, dst):
        """upsample(pyr[dst], pyr[dst+1]), upsample.cu:260-340"""
        src = dst + 1
        w, h, d = self.levels[dst]
        ds = self.levels[src][2]
        factor = 2 if d > ds else 1
        for pg in self.pages[dst]:
            pg.field("v")[...] = 0
        for i in range(ds):
            self.pages[dst][min(i * factor, d - 1)].upsample_from(self.pages[src][i])
        if factor > 1:
            fl = self.flows[dst]
            for i in range(1, d, factor):
                if i == d - 1:
                    continue
                out = np.zeros((h, w, 2), dtype=np.float32)
                a = [np.ascontiguousarray(x, dtype=np.float32) for x in (
                    self.pages[dst][i - 1].field("v"), fl["f0"][i - 1], fl["f1"][i - 1],
                    self.pages[dst][i + 1].field("v"), fl["b0"][i + 1], fl["b1"][i + 1])]
                lib().vmo_temporal_fill(w, h, *[x.ctypes.data for x in a], out.ctypes.data)
                self.pages[dst][i].field("v")[...] = out

    def init_level(self, lvl, P, cons=()):
        for z, pg in enumerate(self.pages[lvl]):
            pg.init(P.ssim_clamp)
            pg.field("temp_ref")[...] = 0          # lvl.temp.ref/mask.fill(0), morph.cu:313-314
            pg.field("temp_mask")[...] = 0
            pg.set_temporal(0, self.factor_d[lvl + 1])
            pg.splat(self.w0, self.h0, self._cons_for(lvl, z, cons))

    def optimize_level(self, lvl, P, max_iter, stats=None):
        """Morph::optimize_level, morph.cu:1353-1441: the middle page, then the two chains outward"""
        d = self.levels[lvl][2]
        pg, fl = self.pages[lvl], self.flows[lvl]
        its = {}
        mid = d // 2
        pg[mid].set_temporal(0, self.factor_d[lvl + 1])
        its[mid] = pg[mid].optimize(P, max_iter, stats)
        for i in range(mid + 1, d):
            pg[i].initialize_temp(pg[i - 1], fl["f0"][i - 1], fl["f1"][i - 1])
            its[i] = pg[i].optimize(P, max_iter, stats)
        for i in range(mid - 1, -1, -1):
            pg[i].initialize_temp(pg[i + 1], fl["b0"][i + 1], fl["b1"][i + 1])
            its[i] = pg[i].optimize(P, max_iter, stats)
        self.iters[lvl] = its
        return its

    def update_result(self, lvl, w0=None, h0=None):
        """CMatchingThread::update_result, MatchingThread.cpp:22-84: the depth0 full-resolution frames
        of level `lvl`'s field -- the two loops of the reference, literally"""
        w0 = int(w0 if w0 is not None else self.w0)
        h0 = int(h0 if h0 is not None else self.h0)
        d = self.levels[lvl][2]
        factor = int(self.factor_d[0] / self.factor_d[lvl + 1])
        vec = [np.zeros((h0, w0, 2), np.float32) for _ in range(self.depth0)]
        for i in range(d):
            vec[min(i * factor, self.depth0 - 1)] = upscale_result(self.pages[lvl][i].field("v"), w0, h0)
        if factor > 1:
            for i in range(d - 1):
                for k in range(1, factor):
                    if i * factor + k >= self.depth0 - 1:
                        continue
                    beg, end = i * factor, min((i + 1) * factor, self.depth0 - 1)
                    fa = np.float32(k) / np.float32(end - beg)
                    out = np.zeros((h0, w0, 2), np.float32)
                    a, b = np.ascontiguousarray(vec[beg]), np.ascontiguousarray(vec[end])
                    lib().vmo_blend_v(out.ctypes.data, a.ctypes.data, b.ctypes.data, float(fa), out.size)
                    vec[i * factor + k] = out
        return vec

    def solve(self, P, max_iter, drop=1.0, cons=(), stats=None):
        """Morph::calculate_halfway_parametrization, morph.cu:150-168"""
        self.coarse_solve(P, cons)
        mi = float(max_iter)
        for el in range(len(self.levels) - 2, -1, -1):
            self.upsample(el)
            self.init_level(el, P, cons)
            self.optimize_level(el, P, mi, stats)
            mi /= drop


# ---- synchronisation stage (oracle/vm_oracle_sync.c) -------------------------------------------

def sync_levels(w, h, d, start_res):
    """[(w, h, d)] of Pyramid::build(video0, video1, f0, f1, start_res), level 0 first"""
    lw, lh, ld = (np.zeros(64, np.int32) for _ in range(3))
    n = lib().vmo_sync_levels(w, h, d, start_res, lw.ctypes.data, lh.ctypes.data, ld.ctypes.data, 64)
    return [(int(lw[i]), int(lh[i]), int(ld[i])) for i in range(n)]


def sync_row(x, y, z, w, h, d, w_tps, ui=0.0):
    out = np.zeros((5, 5, 5), np.float32)
    lib().vmo_sync_row(x, y, z, w, h, d, w_tps, ui, out.ctypes.data)
    return out


def sync_cons(cons):
    """[(lx, ly, lz, rx, ry, rz)] integer full-resolution positions / frames -> int32 array"""
    return np.ascontiguousarray(np.asarray(cons, np.int32).reshape(-1, 6))


def sync_ui(w, h, d, w0, h0, cons, w_ui):
    c = sync_cons(cons)
    out = [np.zeros((d, h, w), np.float32) for _ in range(4)]
    lib().vmo_sync_ui(w, h, d, w0, h0, c.ctypes.data, len(c), w_ui, *[o.ctypes.data for o in out])
    return out


def sync_diag(ui, w_tps):
    d, h, w = ui.shape
    out = np.zeros_like(ui)
    lib().vmo_sync_diag(w, h, d, w_tps, np.ascontiguousarray(ui).ctypes.data, out.ctypes.data)
    return out


def sync_dot(a, b):
    d, h, w = a.shape
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return float(lib().vmo_sync_dot(a.ctypes.data, b.ctypes.data, w, h, d))


def sync_apply(ui, w_tps, p):
    d, h, w = p.shape
    out = np.zeros_like(p, dtype=np.float32)
    ui = np.ascontiguousarray(ui, np.float32); p = np.ascontiguousarray(p, np.float32)
    lib().vmo_sync_apply(w, h, d, w_tps, ui.ctypes.data, p.ctypes.data, out.ctypes.data)
    return out


def sync_solve_level(x, y, z, w0, h0, cons, w_ui, w_tps, max_iter):
    """in place on x, y, z (d, h, w float32); returns (loop iterations, residual norms^2)"""
    d, h, w = x.shape
    c = sync_cons(cons)
    res = np.zeros(3, np.float32)
    k = lib().vmo_sync_solve_level(w, h, d, w0, h0, c.ctypes.data, len(c), w_ui, w_tps, max_iter,
                                   x.ctypes.data, y.ctypes.data, z.ctypes.data, res.ctypes.data)
    return k, res


def sync_upsample(src, dw, dh, ratio):
    sh, sw = src.shape
    src = np.ascontiguousarray(src, np.float32)
    out = np.zeros((dh, dw), np.float32)
    lib().vmo_sync_upsample(out.ctypes.data, dw, dh, src.ctypes.data, sw, sh, ratio)
    return out


def sync_solve(levels, cons, w_ui, w_tps, max_iter):
    """CSyncThread::run, SyncThread.cpp:58-84: coarsest level from zero, then upsample + solve,
    max_iter * 10 halved per level.  levels as sync_levels() gives them.  Returns (X, Y, Z) of
    level 1."""
    w0, h0, _ = levels[0]
    mi = np.float32(max_iter * 10)
    prev = None
    for el in range(len(levels) - 1, 0, -1):
        w, h, d = levels[el]
        cur = [np.zeros((d, h, w), np.float32) for _ in range(3)]
        if prev is not None:
            pw, ph = levels[el + 1][0], levels[el + 1][1]
            ratios = (np.float32(w) / np.float32(pw), np.float32(h) / np.float32(ph), np.float32(1.0))
            for c in range(3):
                for i in range(d):
                    cur[c][i] = sync_upsample(prev[c][i], w, h, float(ratios[c]))
        sync_solve_level(cur[0], cur[1], cur[2], w0, h0, cons, w_ui, w_tps, float(mi))
        prev = cur
        mi = np.float32(mi / np.float32(2))
    return prev


def sync_result(X, Y, Z, w0, h0):
    """one frame: (h, w) x 3 -> (h0, w0, 4)"""
    h, w = X.shape
    out = np.zeros((h0, w0, 4), np.float32)
    a = [np.ascontiguousarray(t, np.float32) for t in (X, Y, Z)]
    lib().vmo_sync_result(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, w, h, w0, h0, out.ctypes.data)
    return out


def render_resample(vec, video0, video1, forw0, forw1, fa, frame):
    """vec (h, w, 4) f32; video* (d, h, w, 4) u8; forw* (d, h, w, 2) f32 -> (h, w, 3) u8"""
    d, h, w = video0.shape[:3]
    out = np.zeros((h, w, 3), np.uint8)
    a = [np.ascontiguousarray(vec, np.float32), np.ascontiguousarray(video0, np.uint8),
         np.ascontiguousarray(video1, np.uint8), np.ascontiguousarray(forw0, np.float32),
         np.ascontiguousarray(forw1, np.float32)]
    lib().vmo_render_resample(out.ctypes.data, w, h, d, fa, frame, *[t.ctypes.data for t in a])
    return out
