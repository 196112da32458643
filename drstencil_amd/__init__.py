"""drstencil_amd -- MI355X-native DRStencil: Python front end over libdrstencil_amd.so.

The product is the C++ generator (`bin/drstencil`, emits HIP for gfx950) and the C-ABI
runtime in libdrstencil_amd.so (include/drstencil_amd.h).  This module is the thin
ctypes binding used by the tests, the tuner, bench.py and the multi-GPU driver.  It
fails loudly when the native library is missing; there is no CPU or PyTorch fallback.
"""
import ctypes
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdrstencil_amd.so")
ROOT = os.path.dirname(_HERE)
CLI_PATH = os.path.join(ROOT, "bin", "drstencil")
SUPPORT_DIR = os.path.join(_HERE, "csrc", "support")
BENCH_DIR = os.path.join(ROOT, "benchmarks")

_lib = None


class Operands(ctypes.Structure):
    """drs_operands of include/drstencil_amd.h: every array a launch takes beside in and out (device addresses; None where the kernel takes none)."""
    _fields_ = [("size", ctypes.c_size_t), ("src", ctypes.c_void_p), ("res", ctypes.c_void_p), ("fix", ctypes.c_void_p), ("scale", ctypes.c_void_p),
                ("coef", ctypes.c_void_p)]


class NativeLibraryMissing(RuntimeError):
    pass


def lib():
    """Load libdrstencil_amd.so (built by `make -C drstencil_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            "%s not found: build it with `make -C %s` (or __graft_entry__.build()); "
            "drstencil_amd has no fallback path" % (LIB_PATH, os.path.join(_HERE, "csrc")))
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    cpp = ctypes.POINTER(ctypes.c_char_p)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.drs_version.restype = ctypes.c_char_p
    L.drs_free.argtypes = [vp]
    L.drs_generate.argtypes = [ci, cpp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.drs_spec_open.restype = vp
    L.drs_spec_open.argtypes = [ctypes.c_char_p, ci, ci, ci, ci, ctypes.POINTER(ci)]
    L.drs_spec_close.argtypes = [vp]
    for n in ("halo", "dist", "range", "npoints", "iterations", "launches"):
        getattr(L, "drs_spec_" + n).argtypes = [vp]
    L.drs_spec_dims.argtypes = [vp] + [ctypes.POINTER(ci)] * 3
    L.drs_spec_point.argtypes = [vp, ci] + [ctypes.POINTER(ci)] * 3 + [ctypes.POINTER(ctypes.c_double), ctypes.c_char_p]
    L.drs_spec_partition.argtypes = [vp, ctypes.POINTER(ci * 4)]
    L.drs_kernel_build.restype = vp
    L.drs_kernel_build.argtypes = [ci, cpp, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.drs_kernel_close.argtypes = [vp]
    L.drs_kernel_unload.argtypes = [vp]
    L.drs_kernel_info.restype = ctypes.c_char_p
    L.drs_kernel_info.argtypes = [vp]
    L.drs_kernel_path.restype = ctypes.c_char_p
    L.drs_kernel_path.argtypes = [vp]
    L.drs_kernel_resources.restype = ctypes.c_char_p
    L.drs_kernel_resources.argtypes = [vp]
    L.drs_kernel_pair_layout.restype = ctypes.c_int
    L.drs_kernel_pair_layout.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    L.drs_kernel_launch.argtypes = [vp, vp, vp, vp]
    L.drs_kernel_launch_gold.argtypes = [vp, vp, vp, vp]
    L.drs_kernel_launch_pair.argtypes = [vp, vp, vp, vp, vp, vp]
    L.drs_kernel_wrap.argtypes = [vp, vp, vp]
    L.drs_kernel_run.argtypes = [vp, vp, vp, ci, ci, vp]
    L.drs_kernel_run_timed.argtypes = [vp, vp, vp, ci, ci, vp, ctypes.POINTER(ctypes.c_float)]
    L.drs_kernel_launch_src.argtypes = [vp, vp, vp, vp, vp]
    L.drs_kernel_launch_gold_src.argtypes = [vp, vp, vp, vp, vp]
    L.drs_kernel_run_src.argtypes = [vp, vp, vp, vp, ci, ci, vp]
    L.drs_kernel_run_timed_src.argtypes = [vp, vp, vp, vp, ci, ci, vp, ctypes.POINTER(ctypes.c_float)]
    L.drs_kernel_residual_elems.restype = ctypes.c_long
    L.drs_kernel_residual_elems.argtypes = [vp]
    L.drs_kernel_launch_res.argtypes = [vp, vp, vp, vp, vp, vp]
    L.drs_kernel_run_res.argtypes = [vp, vp, vp, vp, vp, ci, vp]
    L.drs_kernel_run_timed_res.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, ctypes.POINTER(ctypes.c_float)]
    L.drs_kernel_launch_fix.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.drs_kernel_launch_gold_fix.argtypes = [vp, vp, vp, vp, vp, vp]
    L.drs_kernel_run_fix.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp]
    L.drs_kernel_run_timed_fix.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, ctypes.POINTER(ctypes.c_float)]
    L.drs_kernel_solve_fix.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_double, ci, ci, vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double)]
    op = ctypes.POINTER(Operands)
    L.drs_kernel_launch_ops.argtypes = [vp, vp, vp, op, vp]
    L.drs_kernel_launch_gold_ops.argtypes = [vp, vp, vp, op, vp]
    L.drs_kernel_run_ops.argtypes = [vp, vp, vp, op, ci, ci, vp]
    L.drs_kernel_run_timed_ops.argtypes = [vp, vp, vp, op, ci, ci, vp, ctypes.POINTER(ctypes.c_float)]
    L.drs_kernel_solve_ops.argtypes = [vp, vp, vp, op, ctypes.c_double, ci, ci, vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double)]
    L.drs_kernel_coef_taps.argtypes = [vp]
    L.drs_kernel_coef_taps.restype = ctypes.c_char_p
    L.drs_kernel_residual.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_double)]
    L.drs_kernel_solve.argtypes = [vp, vp, vp, vp, vp, ctypes.c_double, ci, ci, vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double)]
    L.drs_slab_unique_id.argtypes = [vp]
    L.drs_slab_open.restype = vp
    L.drs_slab_open.argtypes = [ci, cpp, ci, cpp, ci, ci, ci, ci, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.drs_slab_plan.argtypes = [vp, ctypes.POINTER(ctypes.c_long * 8)]
    L.drs_slab_connect.argtypes = [vp, vp, vp]
    L.drs_slab_run.argtypes = [vp, vp, vp, ci]
    L.drs_slab_sync.argtypes = [vp]
    L.drs_slab_stream.restype = vp
    L.drs_slab_stream.argtypes = [vp]
    L.drs_slab_info.restype = ctypes.c_char_p
    L.drs_slab_info.argtypes = [vp]
    L.drs_slab_error.restype = ctypes.c_char_p
    L.drs_slab_error.argtypes = [vp]
    L.drs_slab_close.argtypes = [vp]
    L.drs_fill_random_f64.argtypes = [vp, ctypes.c_size_t, ctypes.c_uint]
    L.drs_fill_random_f32.argtypes = [vp, ctypes.c_size_t, ctypes.c_uint]
    for n in ("drs_check_error_f64", "drs_check_error_f32"):
        f = getattr(L, n)
        f.restype = ctypes.c_double
        f.argtypes = [ci] * 5 + [vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double)]
    _lib = L
    return L


EXPORTS = [
    "drs_version", "drs_free", "drs_generate",
    "drs_spec_open", "drs_spec_close", "drs_spec_halo", "drs_spec_dist", "drs_spec_range", "drs_spec_npoints",
    "drs_spec_iterations", "drs_spec_launches", "drs_spec_dims", "drs_spec_point", "drs_spec_partition",
    "drs_kernel_build", "drs_kernel_close", "drs_kernel_unload", "drs_kernel_info", "drs_kernel_path", "drs_kernel_resources", "drs_kernel_pair_layout", "drs_kernel_launch", "drs_kernel_launch_pair",
    "drs_kernel_wrap", "drs_kernel_launch_gold", "drs_kernel_run", "drs_kernel_run_timed",
    "drs_kernel_launch_src", "drs_kernel_launch_gold_src", "drs_kernel_run_src", "drs_kernel_run_timed_src",
    "drs_kernel_residual_elems", "drs_kernel_launch_res", "drs_kernel_run_res", "drs_kernel_run_timed_res", "drs_kernel_residual", "drs_kernel_solve",
    "drs_kernel_launch_fix", "drs_kernel_launch_gold_fix", "drs_kernel_run_fix", "drs_kernel_run_timed_fix", "drs_kernel_solve_fix",
    "drs_kernel_launch_ops", "drs_kernel_launch_gold_ops", "drs_kernel_run_ops", "drs_kernel_run_timed_ops", "drs_kernel_solve_ops",
    "drs_kernel_coef_taps",
    "drs_fill_random_f64", "drs_fill_random_f32", "drs_check_error_f64", "drs_check_error_f32",
    "drs_slab_unique_id", "drs_slab_open", "drs_slab_plan", "drs_slab_connect", "drs_slab_run", "drs_slab_sync", "drs_slab_stream", "drs_slab_info",
    "drs_slab_error", "drs_slab_close",
]


def _argv(args):
    arr = (ctypes.c_char_p * len(args))(*[os.fsencode(str(a)) for a in args])
    return len(args), arr


def _take(ptr):
    if not ptr or not ptr.value:
        return None
    s = ctypes.string_at(ptr.value).decode()
    lib().drs_free(ptr.value)
    return s


def generate(args):
    """The `drstencil` command as a function (main.cpp:10-280): returns (exit_code, stdout, source|None)."""
    n, arr = _argv(args)
    src, msg = ctypes.c_void_p(), ctypes.c_void_p()
    rc = lib().drs_generate(n, arr, ctypes.byref(src), ctypes.byref(msg))
    return rc, _take(msg) or "", _take(src)


class Spec:
    """Parsed + fused stencil with reuse analysis (DRStencil / DRStencil_2d classes)."""

    def __init__(self, stc_path, ndim, step=1, dist=0, merge_forward=5):
        st = ctypes.c_int()
        self.h = lib().drs_spec_open(os.fsencode(stc_path), ndim, step, dist, merge_forward, ctypes.byref(st))
        self.status = st.value
        if not self.h:
            raise IOError("Error opening stencil file.")
        self.ndim, self.step = ndim, step

    def close(self):
        try:
            if getattr(self, "h", None):
                lib().drs_spec_close(self.h)
                self.h = None
        except Exception:   # interpreter shutdown
            pass

    __del__ = close

    halo = property(lambda s: lib().drs_spec_halo(s.h))
    dist = property(lambda s: lib().drs_spec_dist(s.h))
    range = property(lambda s: lib().drs_spec_range(s.h))
    npoints = property(lambda s: lib().drs_spec_npoints(s.h))
    iterations = property(lambda s: lib().drs_spec_iterations(s.h))
    launches = property(lambda s: lib().drs_spec_launches(s.h))

    @property
    def dims(self):
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib().drs_spec_dims(self.h, a, b, c)
        return a.value, b.value, c.value

    @property
    def shape(self):
        return self.dims if self.ndim == 3 else self.dims[1:]

    @property
    def points(self):
        out = []
        k, j, i, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        buf = ctypes.create_string_buffer(32)
        for p in range(self.npoints):
            lib().drs_spec_point(self.h, p, k, j, i, c, buf)
            out.append(((k.value, j.value, i.value), c.value, buf.value.decode()))
        return out

    @property
    def partition(self):
        a = (ctypes.c_int * 4)()
        lib().drs_spec_partition(self.h, ctypes.byref(a))
        return tuple(a)


class KernelBuildError(RuntimeError):
    pass


class ToleranceHorizonExceeded(RuntimeError):
    """drs_kernel_run / drs_kernel_run_timed returned -3: a temporal (reassociated) kernel was asked for more iterations than it keeps
    the 1e-6 (fp32) / 1e-12 (fp64) tolerance for (include/drstencil_amd.h)."""


class Kernel:
    """A generated kernel: drstencil options -> HIP source -> hipcc (gfx950) -> loaded.

    `args` are exactly the `drstencil` command-line arguments (ending with the .stc path).
    Buffers are raw device pointers (ints), e.g. torch.Tensor.data_ptr().

    Lifetime of the plugin (the compiled .so): a Kernel that is garbage-collected or close()d releases its handle only
    (drs_kernel_close) -- the shared object STAYS MAPPED and its code object stays registered with the HIP runtime for the life of
    the process, so a long-lived process that builds a few kernels never pays for reloading, and launches still in flight are safe.
    unload() (drs_kernel_unload) synchronises the device and dlcloses the plugin: that is what sweeps over thousands of kernels
    (the tuner, the fuzzers) call after each measurement.  Nothing is unmapped implicitly."""

    def __init__(self, args, cache_dir=None):
        n, arr = _argv(args)
        log = ctypes.c_void_p()
        self.h = lib().drs_kernel_build(n, arr, os.fsencode(cache_dir) if cache_dir else None, ctypes.byref(log))
        msg = _take(log)
        if not self.h:
            raise KernelBuildError(msg or "kernel build failed")
        self.info = json.loads(lib().drs_kernel_info(self.h).decode())
        self.path = lib().drs_kernel_path(self.h).decode()
        self.resources = json.loads(lib().drs_kernel_resources(self.h).decode() or "{}")   # registers / scratch / LDS per the compiler
        self.args = list(args)

    # the arrays a launch takes beside in and out, in the order of drs_operands: (keyword d_<name>, the Kernel property that says whether the
    # kernel takes it, the option that makes it, what it is)
    _OPERANDS = (("src", "source", "--source", "the source array"),
                 ("res", "residual_elems", "--residual", "an array of residual_elems elements"),
                 ("fix", "dirichlet", "--dirichlet", "the array of held cells"),
                 ("scale", "scale", "--scale", "the array of per-cell factors"),
                 ("coef", "varcoef", "--varcoef", "the array of per-tap coefficients, shape (%d,) + grid"))

    def _operand(self, row, d, who):
        """One array of a call, checked against the kernel: a kernel generated with the array's option needs it, any other kernel takes none."""
        name, taken, option, what = row
        if getattr(self, taken) and not d:
            raise ValueError("%s(): the kernel was generated with %s and needs d_%s, %s" % (who, option, name, what % len(self.coef_taps) if name == "coef" else what))
        if not getattr(self, taken) and d is not None:
            raise ValueError("%s(): d_%s given, but the kernel was generated without %s" % (who, name, option))
        return d

    def _ops(self, who, d_src, d_res, d_fix, d_scale, d_coef, gold=False):
        """The operand block (drs_operands) of a call, every array checked against the kernel (the gold kernel computes no residual: its block
        holds none).  Every launch of every kind of kernel goes through the operand-block entry points (drs_kernel_*_ops)."""
        arrays = (d_src, d_res, d_fix, d_scale, d_coef)
        return ctypes.byref(Operands(ctypes.sizeof(Operands), *[None if gold and r[0] == "res" else self._operand(r, d, who) for r, d in zip(self._OPERANDS, arrays)]))

    @property
    def varcoef(self):
        """True for kernels generated with --varcoef: a launch takes one more read-only array d_coef of the grid's dtype and shape
        (T,) + grid, T = len(coef_taps), and computes v = sum_t coef[t][p] * in[p + d_t] as the kernel's FMA chain, the array value in the
        constant's place, in front of every other option's operation.  launch, launch_gold, run, run_timed and solve then need the keyword
        d_coef, the same array for every launch of a loop; such a kernel runs through the operand-block entry points (drs_kernel_*_ops)."""
        return bool(self.info.get("varcoef", 0))

    @property
    def coef_taps(self):
        """The taps of a --varcoef kernel as (k, j, i) offsets, in the order of d_coef's grids (k = 0 in 2D); () for any other kernel."""
        return tuple(tuple(t) for t in self.info.get("coef_taps", ()))

    @property
    def scale(self):
        """True for kernels generated with --scale: a launch takes one more read-only array d_scale (w) of the grid's shape and dtype and
        computes v = w * S(in) -- with --scale-centre c, v = C * in + w * S(in) -- in front of - out_old, + src and the --dirichlet select,
        every operation rounded once.  launch, launch_gold, run, run_timed and solve then need the keyword d_scale, the same array for every
        launch of a loop; such a kernel runs through the operand-block entry points (drs_kernel_*_ops)."""
        return bool(self.info.get("scale", 0))

    @property
    def scale_centre(self):
        """The centre coefficient C of a --scale kernel as the emitted source writes it (0.0: no centre term, also for kernels without --scale)."""
        return float(self.info.get("scale_centre", 0))

    @property
    def dirichlet(self):
        """True for kernels generated with --dirichlet: a launch takes one more read-only array d_fix of the grid's shape and dtype and
        stores out = fix wherever fix is not NaN (a held cell, bit for bit), else the value the kernel would store without the option (a free
        cell).  launch, launch_gold, run, run_timed and solve then need the keyword d_fix, the same array for every launch of a loop."""
        return bool(self.info.get("dirichlet", 0))

    @property
    def residual_elems(self):
        """Elements of the residual array of a kernel generated with --residual max (1 + launched workgroups, of the grid's dtype; every
        launch writes all of them, the caller initialises none); 0 for a kernel without the option.  launch, run and run_timed of such a
        kernel need the keyword d_res; d_res[0] then holds the last launch's max |out - in| over the interior (residual())."""
        return int(lib().drs_kernel_residual_elems(self.h))

    def residual(self, d_res):
        """d_res[0] of a --residual kernel as a Python float (the device is synchronised by the copy): the residual of the last launch."""
        if not self._operand(self._OPERANDS[1], d_res, "residual"):
            raise ValueError("residual(): the kernel was generated without --residual")
        v = ctypes.c_double()
        if lib().drs_kernel_residual(self.h, d_res, ctypes.byref(v)) != 0:
            raise RuntimeError("HIP error reading the residual")
        return float(v.value)

    def solve(self, d_a, d_b, d_res, tol, max_launches, check_every=8, d_src=None, stream=0, d_fix=None, d_scale=None, d_coef=None):
        """Run to tolerance (drs_kernel_solve_ops): ping-pong pairs k(A,B); k(B,A), `check_every` pairs between two looks at the residual, until
        it is <= tol.  (status, launches, residual): status 0 converged, 1 max_launches (rounded down to an even number) reached, -4 the
        residual is NaN or inf (a diverged or overflowed run).  The answer is in A."""
        n, r = ctypes.c_int(), ctypes.c_double()
        rc = lib().drs_kernel_solve_ops(self.h, d_a, d_b, self._ops("solve", d_src, d_res, d_fix, d_scale, d_coef), tol, max_launches, check_every, stream,
                                        ctypes.byref(n), ctypes.byref(r))
        if rc == -2:
            raise ValueError("solve(): the kernel was generated without --residual, or check_every < 1")
        if rc == -1:
            raise RuntimeError("HIP error in drs_kernel_solve")
        return rc, n.value, r.value

    def launch(self, d_in, d_out, stream=0, d_src=None, d_res=None, d_fix=None, d_scale=None, d_coef=None):
        rc = lib().drs_kernel_launch_ops(self.h, d_in, d_out, self._ops("launch", d_src, d_res, d_fix, d_scale, d_coef), stream)
        if rc != 0:
            raise RuntimeError("HIP launch error %d" % rc)


    def launch_pair(self, d_in0, d_out0, d_in1, d_out1, stream=0):
        """One launch over two (in, out) pairs (kernels generated with --pair-launch 1)."""
        rc = lib().drs_kernel_launch_pair(self.h, d_in0, d_out0, d_in1, d_out1, stream)
        if rc != 0:
            raise RuntimeError("pair launch error %d (-2: kernel built without --pair-launch 1)" % rc)

    @property
    def periodic(self):
        """True for kernels generated with --boundary periodic (every axis periodic, however spelled)."""
        return self.info.get("boundary") == "periodic"

    @property
    def boundaries(self):
        """The boundary mode of every axis, outermost first: a tuple of "fixed" | "periodic" | "reflect" ((z, y, x) in 3D, (y, x) in 2D),
        from either form of the kernel info ("boundaries" for reflecting and mixed kernels, "boundary" alone for periodic, neither for
        fixed)."""
        if "boundaries" in self.info:
            return tuple(self.info["boundaries"])
        return (self.info.get("boundary", "fixed"),) * self.info["ndim"]

    @property
    def fills_ring(self):
        """True when some axis is not fixed: every launch first fills the input's ring on those axes from its interior (wrap())."""
        return any(m != "fixed" for m in self.boundaries)

    @property
    def time_order(self):
        """2 for kernels generated with --time-order 2: a launch computes out = S(in) - out_old on the interior, so the output array's
        interior is input too (the ping-pong loop of run() is then the leapfrog scheme u(t+1) = S(u(t)) - u(t-1)); else 1."""
        return int(self.info.get("time_order", 1))

    @property
    def source(self):
        """True for kernels generated with --source: a launch takes a third, read-only array d_src of the grid's shape and computes
        out = S(in) + src on the interior (with --time-order 2: (S(in) - out_old) + src); launch, launch_gold, run and run_timed then
        need the keyword d_src, the same array for every launch of a loop."""
        return bool(self.info.get("source", 0))

    def wrap(self, d, stream=0):
        """Kernels with a non-fixed axis (--boundary periodic | reflect, --boundary-x / -y / -z): fill the ring of width Halo of the device
        array `d` on those axes from its interior (periodic images one period, dim - 2 Halo, away; zero-flux mirror images about the face
        between ring and interior), asynchronously on `stream`.  The ring of a fixed axis is not written.  Every launch does this to its
        input first."""
        rc = lib().drs_kernel_wrap(self.h, d, stream)
        if rc == -2:
            raise RuntimeError("wrap(): the kernel fills no ring (every axis is fixed: generate it with --boundary periodic | reflect or a per-axis --boundary-x / -y / -z)")
        if rc != 0:
            raise RuntimeError("HIP launch error %d" % rc)

    def launch_gold(self, d_in, d_out, stream=0, d_src=None, d_fix=None, d_scale=None, d_coef=None):
        rc = lib().drs_kernel_launch_gold_ops(self.h, d_in, d_out, self._ops("launch_gold", d_src, None, d_fix, d_scale, d_coef, gold=True), stream)
        if rc != 0:
            raise RuntimeError("HIP launch error %d" % rc)

    def run(self, d_a, d_b, iterations=None, gold=False, stream=0, d_src=None, d_res=None, d_fix=None, d_scale=None, d_coef=None):
        """The reference's ping-pong loop (codegen.hpp:581-584); result ends in A.  --source kernels: the same d_src in every launch.
        --residual kernels: d_res[0] then holds the last launch's residual (the gold kernel computes none: gold=True takes no d_res)."""
        it = self.info["iterations"] if iterations is None else iterations
        if gold and d_res is not None:
            raise ValueError("run(): the gold kernel computes no residual")
        n = lib().drs_kernel_run_ops(self.h, d_a, d_b, self._ops("run", d_src, d_res, d_fix, d_scale, d_coef, gold=gold), it, 1 if gold else 0, stream)
        if n == -3:
            raise ToleranceHorizonExceeded(self._horizon_message(it))
        if n < 0:
            raise RuntimeError("HIP error in drs_kernel_run")
        return n


    def check_slabs(self, nsl):
        """Where a checker should look: [(label, first slice)] of `nsl`-slice slabs of the outermost dimension -- the bottom of the grid, a slab
        ACROSS a stream-block (z-streaming / row-streaming kernels) or tile-row (one-shot 2D tiles) boundary in the middle, where two
        workgroups' ownership meets, and the top, where byte offsets are largest (beyond 2^32 at 1024^3).  The caller runs its reference
        (the CPU oracle in tests/ and bench.py's cpu_baseline leg) on in[z0 : z0 + nsl] and compares out[z0 + Halo : z0 + nsl - Halo]."""
        i = self.info
        dim0 = i["L"] if i["ndim"] == 3 else i["M"]
        nsl = min(nsl, dim0)
        if i.get("streams", 1):
            edge = i["halo"] + (i.get("stream_blocks", 1) // 2) * i.get("sn", dim0)       # first output slice of the middle stream block
        else:
            edge = (i.get("tiles_y", 1) // 2) * i.get("tile_owned_rows", dim0)             # first row of the middle tile row
        if not (i["halo"] < edge < dim0 - i["halo"]):
            edge = dim0 // 2
        mid = max(0, min(dim0 - nsl, edge - nsl // 2))
        out = [("bottom", 0)]
        if mid > 0 and mid < dim0 - nsl:
            out.append(("block_boundary", mid))
        if dim0 - nsl > 0:
            out.append(("top", dim0 - nsl))
        return out

    def run_timed(self, d_a, d_b, iterations=None, warmup=10, stream=0, d_src=None, d_res=None, d_fix=None, d_scale=None, d_coef=None):
        """Warm-up launches + timed loop bracketed by HIP events on `stream`: (launches, ms)."""
        it = self.info["iterations"] if iterations is None else iterations
        ms = ctypes.c_float()
        n = lib().drs_kernel_run_timed_ops(self.h, d_a, d_b, self._ops("run_timed", d_src, d_res, d_fix, d_scale, d_coef), it, warmup, stream, ctypes.byref(ms))
        if n == -3:
            raise ToleranceHorizonExceeded(self._horizon_message(it))
        if n < 0:
            raise RuntimeError("HIP error in drs_kernel_run_timed")
        return n, ms.value


    def _horizon_message(self, it):
        return ("%d iterations exceed the tolerance horizon (%d) of this reassociated (temporal) kernel: build the fused kernel, or pass "
                "--temporal force" % (it, self.info.get("tolerance_horizon_iterations", -1)))

    # work / traffic model
    def updates_per_launch(self):
        i = self.info
        h = i["halo"]
        dims = [i["L"], i["M"], i["N"]] if i["ndim"] == 3 else [i["M"], i["N"]]
        n = 1
        for d in dims:
            n *= d - 2 * h
        return n * i["step"]

    def bytes_per_launch(self):
        i = self.info
        pts = i["M"] * i["N"] * (i["L"] if i["ndim"] == 3 else 1)
        # --time-order 2 also reads the old output, --source the source array: one more whole array each is the algorithmic minimum (the centre
        # values of --residual are cells the sweep reads anyway)
        # --dirichlet reads the array of held cells: one more whole array
        # --scale reads the array of factors: one more whole array (the centre values of --scale-centre are cached re-reads, as --residual's)
        # --varcoef reads the T coefficient grids: T more whole arrays
        return (2 + (self.time_order == 2) + self.source + self.dirichlet + self.scale + len(self.coef_taps)) * (4 if i["dtype"] == "fp32" else 8) * pts

    # ---- placement of the output array (csrc/schedule.hpp: Schedule::out_skew_bytes; profiles/r03_probe_skew4.log) ----
    def array_bytes(self):
        i = self.info
        return (4 if i["dtype"] == "fp32" else 8) * i["M"] * i["N"] * (i["L"] if i["ndim"] == 3 else 1)

    def pair_layout(self, skew=None):
        """(arena bytes, byte offset of the output array) for both arrays of this kernel in ONE allocation: the output starts
        `skew` bytes (default: the kernel's own recommendation, info["out_skew_bytes"]) past a multiple of the 64 MiB placement
        period behind the input.  A z-streaming kernel's launch time depends on (out - in) mod 64 MiB by up to 14 %."""
        period = int(self.info.get("placement_period_bytes", 64 << 20))
        skew = int(self.info.get("out_skew_bytes", 0)) if skew is None else int(skew)
        nb = self.array_bytes()
        off = -(-nb // period) * period + skew % period
        return off + nb, off

    def alloc_pair(self, torch, device, dtype=None, skew=None, calibrate=False, stream=0):
        """Both arrays of the kernel's grid as views of one torch allocation laid out by pair_layout(): (A, B, arena).  With
        calibrate=True the skew is MEASURED on this device instead (both directions of the ping-pong at eight positions, a few
        launches each, contents undefined afterwards) -- the kernel's recommendation is a model, the arena has room for any skew."""
        i = self.info
        dtype = dtype or (torch.float32 if i["dtype"] == "fp32" else torch.float64)
        shape = (i["L"], i["M"], i["N"]) if i["ndim"] == 3 else (i["M"], i["N"])
        period = int(i.get("placement_period_bytes", 64 << 20))
        nb = self.array_bytes()
        base_off = -(-nb // period) * period
        arena = torch.empty(base_off + period + nb, dtype=torch.uint8, device=device)
        if calibrate:
            arena.zero_()
            skew, table = self.calibrate_skew(torch, arena.data_ptr(), arena.data_ptr() + base_off, period, stream=stream)
            self.skew_calibration = table
        elif skew is None:
            skew = int(i.get("out_skew_bytes", 0))
        off = base_off + int(skew) % period
        n = nb // arena.new_empty(0, dtype=dtype).element_size()
        A = arena[:nb].view(dtype).view(shape)
        B = arena[off:off + nb].view(dtype).view(shape)
        assert A.numel() == n and B.data_ptr() - A.data_ptr() == off
        self.pair_skew_bytes = int(skew) % period
        return A, B, arena

    def calibrate_skew(self, torch, d_in, d_out0, period, steps=4, launches=4, stream=0):
        """Time in -> out and out -> in for out = d_out0 + j * period / steps on torch's current stream; returns (best skew in bytes,
        [(skew, ms fwd, ms bwd)]).  Four positions, 16 MiB apart: kernels with several z fronts in flight (16 MiB apart for the full-row
        step-1 kernel) dislike odd multiples of 8 MiB, and the single-front kernels' good zone is 24 MiB wide (profiles/r03_probe_skew5.log).
        A position within 0.5 % of the best that equals the kernel's own recommendation wins (noise must not move it).  (`stream` is
        accepted for symmetry with launch() and ignored: the events and the launches must share a stream, and that is the current one.)"""
        st = torch.cuda.current_stream()
        s = st.cuda_stream
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        table = []
        for _ in range(12):                              # clocks up before the first position is timed (it would look slow otherwise)
            self.launch(d_in, d_out0 + period // 2, s); self.launch(d_out0 + period // 2, d_in, s)
        for j in range(steps):
            d_out = d_out0 + j * (period // steps)
            self.launch(d_in, d_out, s); self.launch(d_out, d_in, s)
            e[0].record(st)
            for _ in range(launches):
                self.launch(d_in, d_out, s)
            e[1].record(st)
            for _ in range(launches):
                self.launch(d_out, d_in, s)
            e[2].record(st)
            torch.cuda.synchronize()
            table.append((j * (period // steps), e[0].elapsed_time(e[1]) / launches, e[1].elapsed_time(e[2]) / launches))
        best = min(table, key=lambda r: r[1] + r[2])
        rec = int(self.info.get("out_skew_bytes", 0)) % period
        for r in table:
            if r[0] == rec and r[1] + r[2] <= 1.005 * (best[1] + best[2]):
                best = r
        return best[0], table

    def close(self):
        """Release the handle; the plugin stays mapped (see the class docstring)."""
        try:
            if getattr(self, "h", None):
                lib().drs_kernel_close(self.h)
                self.h = None
        except Exception:   # interpreter shutdown
            pass

    def unload(self):
        """close() and unmap the plugin (device synchronised first): sweeps over thousands of kernels."""
        if getattr(self, "h", None):
            h, self.h = self.h, None
            if lib().drs_kernel_unload(h) != 0:
                raise RuntimeError("drs_kernel_unload failed")

    __del__ = close


def slab_unique_id():
    """The 128-byte id a slab communicator is created from (rank 0 calls this and distributes the bytes)."""
    buf = ctypes.create_string_buffer(128)
    if lib().drs_slab_unique_id(buf) != 0:
        raise RuntimeError("drs_slab_unique_id failed (librccl not found?)")
    return buf.raw


class Slab:
    """One rank of a slab-decomposed run through the native N > 1 entry points (include/drstencil_amd.h: drs_slab_*): plan and
    kernels in the constructor (before any GPU call), connect() once the device is set, run() on caller-owned device buffers of
    `Lloc` planes.  multigpu.SlabRun is the torch.distributed implementation it equals bit for bit."""

    def __init__(self, args, world, rank, every=1, alone_args=None, rehearse_world=0, cache_dir=None):
        n, arr = _argv(args)
        an, aarr = _argv(alone_args) if alone_args else (0, None)
        log = ctypes.c_void_p()
        self.h = lib().drs_slab_open(n, arr, an, aarr, world, rank, every, rehearse_world, os.fsencode(cache_dir) if cache_dir else None, ctypes.byref(log))
        msg = _take(log)
        if not self.h:
            raise KernelBuildError(msg or "drs_slab_open failed")
        p = (ctypes.c_long * 8)()
        lib().drs_slab_plan(self.h, ctypes.byref(p))
        self.lo, self.hi, self.z0, self.z1, self.Lloc, self.G, self.H, self.every = [int(x) for x in p]

    def connect(self, unique_id, stream=0):
        if lib().drs_slab_connect(self.h, unique_id, stream) != 0:
            raise RuntimeError("drs_slab_connect: " + lib().drs_slab_error(self.h).decode())

    def run(self, d_a, d_b, iterations=-1):
        n = lib().drs_slab_run(self.h, d_a, d_b, iterations)
        if n < 0:
            raise RuntimeError("drs_slab_run: " + lib().drs_slab_error(self.h).decode())
        return n

    def sync(self):
        if lib().drs_slab_sync(self.h) != 0:
            raise RuntimeError("drs_slab_sync failed")

    @property
    def stream(self):
        return lib().drs_slab_stream(self.h)

    @property
    def info(self):
        return json.loads(lib().drs_slab_info(self.h).decode())

    def close(self):
        try:
            if getattr(self, "h", None):
                lib().drs_slab_close(self.h)
                self.h = None
        except Exception:   # interpreter shutdown
            pass

    __del__ = close


def fill_random(arr, seed=1):
    """common.hpp:9-32 input stream into a numpy array (in place)."""
    import numpy as np
    fn = {np.dtype("float64"): lib().drs_fill_random_f64, np.dtype("float32"): lib().drs_fill_random_f32}[arr.dtype]
    fn(arr.ctypes.data, arr.size, seed)
    return arr


def check_error(out, ref, halo):
    """checkError2D/3D (common.hpp:47-102): dict(rms, max_abs, max_idx, max_rel) over the interior."""
    import numpy as np
    assert out.shape == ref.shape and out.dtype == ref.dtype
    nd = out.ndim
    L, M, N = (out.shape if nd == 3 else (1,) + tuple(out.shape))
    fn = {np.dtype("float64"): lib().drs_check_error_f64, np.dtype("float32"): lib().drs_check_error_f32}[out.dtype]
    ma, mi, mr = ctypes.c_double(), ctypes.c_long(), ctypes.c_double()
    rms = fn(nd, L, M, N, halo, out.ctypes.data, ref.ctypes.data, ma, mi, mr)
    return dict(rms=rms, max_abs=ma.value, max_idx=mi.value, max_rel=mr.value)
