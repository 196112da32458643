"""Kernel configurations of the --scale tests (tests/test_scale_cpu.py under the CPU emulation, tests/test_scale_gpu.py on the GPU: the
same list in both places) and of scripts/scale_cost.py, prebuilt by __graft_entry__.build() so that the GPU box finds them in
drstencil_amd/_kcache and no GPU test starts the compiler.  Also what the two suites share: the emulated plugin's loader, the inputs, the
host reference and its contracted variants.

The geometries are tests/residual_cases.py's (EDGE, BIG, its buffer-mask form, the step-1 KNOBS and MODES); the option refuses fused
steps, so those are left out.

The reference of one launch (in -> out), host_launch: the ring fill of the non-fixed axes on `in`, oracle.sweep(..., contract=1) -- the
fused FMA chain rounded once -- and then numpy operations in the array's dtype on the interior I, one rounding each, in the contract's order
    v = w[I] * v;   t = C * in[I]; v = t + v  (centre c != 0);   v = v - out_old[I];   v = v + src[I];   v = where(isnan(fix[I]), v, fix[I])
with C = dtype(float("%g" % c)), the value the emitted source writes.  With --residual max the residual is numpy's max(abs(out[I] - in[I])).

The centre values: 0 (no centre term), 1, 2 and 0.3 (no power of two: the product rounds).  Every geometry of GEOMS runs with one of
them, round robin, and BIG with all four; every MODES entry runs with --scale alone, with --scale-centre 2, and with every option at once
and centre 0.3.

The samples of the tuner's space (sample_jobs): fuzz_parity.make_jobs(20, seed, "order2") with --time-order 2 replaced by --scale, and
make_jobs(20, seed, "order2_source") with --scale --scale-centre 2 appended.  Refusals are decided when build() compiles (the generator
refuses an LDS demand beyond the limit and LDS-DMA staging on rows that are no multiple of the 16-byte vector; the runtime refuses kernels
that spill), so they are known before any GPU run: REFUSED lists them.  Each seed is the first for which at most 5 of the 20 are refused,
cross-compiling for gfx950."""
import ctypes
import hashlib
import os
import subprocess
from fractions import Fraction

import numpy as np

import dirichlet_cases as dc
import residual_cases as rc
from residual_cases import F32, F64, ORDER2, RES, ROOT, SOURCE, dtype_of, interior, residual_of, same_bits, stc  # noqa: F401

SCALE = ["--scale"]
DIR = dc.DIR
CENTRES = (0, 1, 2, 0.3)


def centre_opts(c):
    return ["--scale-centre", repr(c) if isinstance(c, float) else str(c)] if c else []


def with_scale(opts, c=0):
    return list(opts) + SCALE + centre_opts(c)


def centre_of(opts):
    """The centre coefficient of a command line as the emitted source writes it: six significant digits ("%g")."""
    return float("%g" % float(opts[opts.index("--scale-centre") + 1])) if "--scale-centre" in opts else 0.0


EDGE = dc.EDGE                      # min_333 periodic (one interior cell), thin 7x9x13 (branch, buffer, fp64), tile_plus1 (branch, buffer)
BIG = dc.BIG                        # 70 x 45 x 530 with early-leaving workgroups
BIG_BUFFER = dc.BIG_BUFFER
# 2D tile, 2D stream, DMA stream, buffer mask, deferred stores, rows + pack, cyclic merge, loader waves, depth 2, element-wide rows.  The
# fp64 loader-wave kernel runs on 32-column tiles, as in tests/dirichlet_cases.py: at its default 64 columns a third array spills already,
# and the runtime refuses a kernel that spills
# Geometries that spill with the further streams, cross-compiling for gfx950 (the runtime refuses a kernel that spills; that rule stays),
# run on tiles of half as many rows per lane:
#   prefetch_depth2 with a centre term   three sets each of w and of the centre values: 164 bytes of scratch per lane (--scale alone fits)
#   order2_fp32 with a centre term       44 bytes per lane; with every option at once 336
#   reflect_fp32 with every option       one scalar register
_HALF = ["--by", "4", "--block-merge-y", "2"]
SMALLER = {"prefetch_depth2": _HALF, "order2_fp32_centre2": _HALF, "order2_fp32_all_c0.3": _HALF, "reflect_fp32_all_c0.3": _HALF}
KNOBS = [(c[0], c[1], c[2], c[3] + SMALLER.get(c[0], [])) for c in dc.KNOBS]
GEOMS = EDGE + [BIG_BUFFER] + KNOBS
# (id, ndim, spec, options without --scale, centre)
CASES = [(g[0] + "_c%s" % CENTRES[n % 4], g[1], g[2], g[3], CENTRES[n % 4]) for n, g in enumerate(GEOMS)]
CASES += [(BIG[0] + "_c%s" % c, BIG[1], BIG[2], BIG[3], c) for c in CENTRES]
# every mode: --scale alone, --scale-centre 2, and every option at once with centre 0.3 (r after every launch).  All six streams at the
# prefetch distance on the buffer-mask path spill scalar registers (five do already, tests/dirichlet_cases.py): that geometry loads its
# streams in the plane's own iteration
_ALL = ORDER2 + SOURCE + DIR + RES


def _all_of(cid, opts):
    base = [o for n, o in enumerate(opts) if not (o in ("--time-order", "--source") or (n and opts[n - 1] == "--time-order"))]
    if cid == "order2_source_buffer":
        base = [o for o in base if o != "--prefetch"]
    return base + _ALL


MODES = [(c[0] + "_scale", c[1], c[2], c[3], 0) for c in rc.MODES] + [(c[0] + "_centre2", c[1], c[2], c[3], 2) for c in rc.MODES] + \
        [(c[0] + "_all_c0.3", c[1], c[2], _all_of(c[0], c[3]), 0.3) for c in rc.MODES]
MODES = [(c[0], c[1], c[2], c[3][:3] + SMALLER.get(c[0], []) + c[3][3:], c[4]) for c in MODES]
MIN_333 = EDGE[0]
# unit scale: the arrays of the same command without the option (plain kernels prebuilt too)
UNCHANGED = list(rc.UNCHANGED)
# planted factors
PLANT = dc.PLANT
# no contraction: centre 0.3, fp32 and fp64, on BIG and on the 2D tile
TILE2 = [c for c in KNOBS if c[0] == "tile_2d_fp32"][0]


def _as(dtype, c):
    return (c[0] + "_" + dtype, c[1], c[2], [("fp32" if o == "fp64" else o) if dtype == "fp32" else ("fp64" if o == "fp32" else o) for o in c[3]])


CONTRACTION = [_as("fp32", BIG), _as("fp64", BIG), _as("fp32", TILE2), _as("fp64", TILE2)]
# frozen field (w = 0, centre 1) and special values
FROZEN = [BIG, BIG_BUFFER, TILE2]
SPECIAL = dc.PLANT
# the memory contract under PROT_NONE pages: the edge grids and three knob cases
CONTRACT = EDGE + [c for c in KNOBS if c[0] in ("prefetch_depth2", "store_mask_buffer", "stream_2d_fp32")]
# the read log over w: 16-byte rows with partial vectors, element rows, prefetched and DMA-staged streams, the 2D tile, order 2 + source
READLOG = [next((k for k in KNOBS if k[0] == c[0]), c) for c in dc.READLOG]
# guard-band arena on the GPU
ARENA = [next((k for k in KNOBS if k[0] == c[0]), c) for c in dc.ARENA]
# run to tolerance: residual_cases.SOLVE's kernels, tolerances and MAX_LAUNCHES on screened Poisson
SOLVE = rc.SOLVE
SOLVE_DIMS = rc.SOLVE_DIMS
MAX_LAUNCHES = rc.MAX_LAUNCHES
CHECK_PROGRAM = ("3d_scale_check_program", 3, stc("lap3"), ["--3d", "--dtype", "fp64", "--check", "--boundary", "periodic"] + ORDER2 + SOURCE + SCALE + ["--scale-centre", "2"])
LAP3, LAP2 = stc("lap3"), stc("lap2")
# the two README forms on the Laplacians: a heterogeneous heat step and a wave with a velocity model
FORMS = [("heat_lap3_fp32", 3, LAP3, F32, 1), ("heat_lap2_fp64", 2, LAP2, ["--dtype", "fp64"], 1),
         ("wave_lap3_fp64", 3, LAP3, F64 + ORDER2, 2), ("wave_lap2_fp32", 2, LAP2, ["--dtype", "fp32"] + ORDER2, 2)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def inputs(spec, opts, seed=11):
    """(A, B, F or None, fix or None, w): residual_cases' A, B, F; dirichlet_cases' pattern of held cells with --dirichlet; factors of both
    signs and magnitudes up to 1.5."""
    from fuzz_parity import signed_random
    A, B, F = rc.inputs(spec, opts, seed)
    dt = dtype_of(opts)
    X = dc.fix_pattern(spec.shape, dt, seed + 6) if "--dirichlet" in opts else None
    W = (signed_random(spec.shape, dt, seed + 7) * 1.5).astype(dt)
    return A, B, F, X, W


def w_specials(dt):
    """Factors arithmetic treats specially: +0.0, -0.0, +inf, -inf, NaN, the smallest subnormal of either sign."""
    tiny = np.nextafter(np.asarray(0, dt), np.asarray(1, dt))
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny], dt)


def special_problem(spec, opts, info, seed=11):
    """(A, B, F, fix, w, cells) for the special-value test.  w holds every value of w_specials in turn at residual_cases.planted_cells
    (corners and seams).  Three interior sites, far apart along x, are then BUILT (every coefficient of these stencils is positive and the
    centre tap exists):
      zero_times_inf : in[p] = +inf, w[p] = +0.0        -> S(in)[p] = +inf, the scaled value is NaN; with --dirichlet p is held at 0.5
      inf_times_fin  : w[q] = +inf, in finite around q  -> the scaled value is +-inf
      m0_times_m0    : in = -0.0 on the whole neighbourhood of s, w[s] = -0.0 -> S(in)[s] = -0.0
    Whether each site is what it is meant to be is asserted by the tests on the reference alone."""
    A, B, F, X, W = inputs(spec, opts, seed)
    dt = np.dtype(dtype_of(opts))
    H = spec.halo
    sp = w_specials(dt)
    for n, c in enumerate(rc.planted_cells(info)):
        W[c] = sp[n % len(sp)]
    dims = spec.shape
    lo = [H + 1] * 3
    hi = [d - H - 2 for d in dims]
    mid = [(a + b) // 2 for a, b in zip(lo, hi)]
    xs = [lo[2] + 3, mid[2] + 5, hi[2] - 3]
    p, q, s = [(mid[0] + 1, mid[1] + 1, x) for x in xs]
    A[p] = np.inf
    W[p] = 0.0
    W[q] = np.inf
    blk = tuple(slice(c - H, c + H + 1) for c in s)
    A[blk] = -0.0
    W[s] = -0.0
    if F is not None:
        F[blk] = -0.0
    if X is not None:
        nanq = np.asarray(np.nan, dt)
        X[p] = 0.5
        X[q] = nanq
        X[s] = nanq
    return A, B, F, X, W, {"zero_times_inf": p, "inf_times_fin": q, "m0_times_m0": s}


# ---- host reference ------------------------------------------------------------------------------------------------------------------
def plain_opts(opts):
    """The command line without --scale and --scale-centre c."""
    out, skip = [], False
    for o in opts:
        if skip:
            skip = False
        elif o == "--scale-centre":
            skip = True
        elif o != "--scale":
            out.append(o)
    return out


def _fma_exact(a, b, c, dt):
    """round(a * b + c) once, element by element: fp32 through float64 (the product of two fp32 values is exact there), fp64 in rationals."""
    if np.dtype(dt) == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    out = np.empty(a.shape, np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def scaled(v, w, cen, C, variant=None):
    """The contract's scale steps on interior values: v = w * v, then (C != 0) t = C * in; v = t + v.  variant: a CONTRACTED evaluation,
    which the kernel must NOT compute -- "fma_w": v = fma(w, v, t), "fma_c": v = fma(C, in, w * v)."""
    dt = v.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        if C == 0.0:
            return w * v
        Cd = np.full(v.shape, C, dt)
        if variant == "fma_w":
            return _fma_exact(w, v, Cd * cen, dt).astype(dt)
        if variant == "fma_c":
            return _fma_exact(Cd, cen, w * v, dt).astype(dt)
        v = w * v
        t = Cd * cen
        return t + v


def host_launch(spec, ndim, opts, src, dst, F, X, W, variant=None, cells=None):
    """One launch src -> dst of a kernel generated with `opts` (with --scale in them), in place.  Returns the residual of the stored arrays
    (a 0-d array of the dtype).  variant: see scaled().  cells: an interior mask -- the scale steps are evaluated there only and every
    other interior cell of dst is left as it was (the fp64 rationals are slow: a few hundred cells)."""
    import boundary_cases
    import oracle
    H = spec.halo
    modes = boundary_cases.modes_of(list(opts) + ["x"], ndim)
    if any(m != "fixed" for m in modes):
        boundary_cases.host_fill(src, H, modes)
    tmp = dst.copy()
    oracle.sweep(spec, src, tmp, contract=1)
    C = np.asarray(centre_of(opts), src.dtype)[()]
    v, d, cen, w = interior(tmp, H), interior(dst, H), interior(src, H), interior(W, H)
    assert v.dtype == d.dtype == w.dtype == src.dtype
    sel = (slice(None),) * v.ndim if cells is None else cells
    with np.errstate(invalid="ignore", over="ignore"):
        r = scaled(v[sel], w[sel], cen[sel], C, variant)
        if "--time-order" in opts:
            r = r - d[sel]
        if "--source" in opts:
            r = r + interior(F, H)[sel]
        if "--dirichlet" in opts:
            f = interior(X, H)[sel]
            r = np.where(np.isnan(f), r, f)
        assert r.dtype == src.dtype
        d[sel] = r
        return residual_of(src, dst, H)


def oracle_solve(spec, A, B, F, X, W, tol, max_launches, check_every):
    """The run to tolerance as a numpy loop of the host reference that looks at r at the same launches: (status, launches, r)."""
    opts = ["--source"] + (DIR if X is not None else [])
    n, r = 0, None
    limit = max_launches - max_launches % 2
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            for src, dst in ((A, B), (B, A)):
                r = host_launch(spec, 3, opts, src, dst, F, X, W)
                n += 1
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r


def solve_problem(spec, dt, sigma=True, held=False):
    """Screened Poisson -Lap u + sigma u = f on a cube with a ring of 0, as a Jacobi sweep of tests/stc/jacobi3.stc (the average of the six
    neighbours): u' = w * S(u) + src with w = 6 / (6 + sigma), src = f / (6 + sigma).  sigma: a smooth positive field (0 with sigma=False:
    plain Poisson, w = 1); f = 1.  held: an inner block held at 0.25 through fix.  (A, B, src, fix or None, w), everything starting at 0."""
    H = spec.halo
    shape = spec.shape
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) / (n - 1) for n in shape], indexing="ij")
    sig = (1.5 + np.cos(2 * np.pi * g[0]) * np.sin(np.pi * g[1]) * 0.75 + g[2] * 0.5) if sigma else np.zeros(shape)
    assert (sig > 0).all() or not sigma
    W = (6.0 / (6.0 + sig)).astype(dt)
    F = np.zeros(shape, dt)
    interior(F, H)[...] = interior((1.0 / (6.0 + sig)).astype(dt), H)
    A = np.zeros(shape, dt)
    X = None
    if held:
        n = shape[0]
        a, b = n // 2 - n // 8 - 1, n // 2 + n // 8 + 1
        X = np.full(shape, np.nan, dt)
        X[a:b, a:b, a:b] = 0.25
        A[a:b, a:b, a:b] = 0.25
    return A, A.copy(), F, X, W


# ---- the samples of the tuner's space --------------------------------------------------------------------------------------------------
SAMPLES = {"scale": 1, "order2_source_scale_centre2": 1}          # sample -> seed of fuzz_parity.make_jobs
SAMPLE_SIZE = 20
MIN_CHECKED = 15                                                  # at most 5 of 20 refused
# what build() refuses of each sample, cross-compiling for gfx950: (index in the sample, reason)
REFUSED = {"scale": [(12, "--stage dma needs 16-byte vectors: the 2D grid's rows are no multiple of 4 fp32")],
           "order2_source_scale_centre2": [(4, "the tile needs more than 160 KiB of LDS"), (5, "spills 24 bytes per lane to scratch memory"),
                                           (7, "spills 288 bytes per lane to scratch memory")]}


def sample_jobs(which, seed=None):
    """fuzz_parity's tuples (ndim, stc, dtype, args, step) of sample `which`."""
    import fuzz_parity
    seed = SAMPLES[which] if seed is None else seed
    out = []
    if which == "scale":
        for ndim, path, dtype, args, step in fuzz_parity.make_jobs(SAMPLE_SIZE, seed, "order2"):
            a = list(args)
            i = a.index("--time-order")
            a[i:i + 2] = SCALE
            out.append((ndim, path, dtype, a, step))
    else:
        for ndim, path, dtype, args, step in fuzz_parity.make_jobs(SAMPLE_SIZE, seed, "order2_source"):
            out.append((ndim, path, dtype, list(args[:-1]) + SCALE + ["--scale-centre", "2"] + [args[-1]], step))
    return out


# ---- what build() compiles -----------------------------------------------------------------------------------------------------------
def cost_cases():
    """scripts/scale_cost.py: (workload, tuned step-1 options, with --source, with --scale, with --scale --scale-centre 1)."""
    import source_cases
    return [(w, source_cases.step1_tuned(w), source_cases.step1_tuned(w) + SOURCE, with_scale(source_cases.step1_tuned(w)), with_scale(source_cases.step1_tuned(w), 1))
            for w in ("c2", "c4")]


def solve_opts(opts, held=False):
    return with_scale(list(opts) + SOURCE + RES + (DIR if held else []))


def all_build_args():
    out = [with_scale(c[3], c[4]) + [c[2]] for c in CASES + MODES + FORMS]
    out += [with_scale(c[3]) + [c[2]] for c in UNCHANGED] + [list(c[3]) + [c[2]] for c in UNCHANGED]
    out += [with_scale(c[3]) + [c[2]] for c in PLANT]
    out += [with_scale(c[3], 0.3) + [c[2]] for c in CONTRACTION]
    out += [with_scale(c[3], 1) + [c[2]] for c in FROZEN]
    out += [with_scale(c[3], 1) + [c[2]] for c in SPECIAL] + [with_scale(c[3] + DIR, 1) + [c[2]] for c in SPECIAL]
    out += [with_scale(c[3], 2) + [c[2]] for c in ARENA]
    for cid, ndim, src, opts, tol in SOLVE:
        out += [solve_opts(opts) + [src], solve_opts(opts, True) + [src]]
    # the operand block on old kinds of kernel: plain, --source, --dirichlet
    out += [list(o) + [EDGE[1][2]] for o in (EDGE[1][3], EDGE[1][3] + SOURCE, EDGE[1][3] + DIR, EDGE[1][3] + RES)]
    seen, uniq = set(), []
    for a in out:
        if tuple(a) not in seen:
            seen.add(tuple(a))
            uniq.append(a)
    return uniq


def cost_build_args():
    b = rc._bench()
    out = []
    for w, plain, src, scl, cen in cost_cases():
        out += [o + [b.WORKLOADS[w]["stc"]] for o in (plain, src, scl, cen)]
    return out


def check_program_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "emitted_programs", "scale_check")


def build_check_program(drs):
    """Generate and compile the standalone --check --scale program (run by tests/test_scale_gpu.py); called by __graft_entry__.build(), so
    that no test starts hipcc."""
    import shutil
    exe = check_program_path()
    out = os.path.dirname(exe)
    os.makedirs(out, exist_ok=True)
    shutil.copy(os.path.join(drs.SUPPORT_DIR, "common.hpp"), out)
    _, _, src, opts = CHECK_PROGRAM
    subprocess.check_call([drs.CLI_PATH] + opts + ["-o", exe + ".hip", os.path.basename(src)], cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-o", exe, exe + ".hip"])
    return exe


def c_host_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "c_host", "capi_ops_host")


def build_c_host(drs):
    """tests/native/capi_ops_host.c (the INTEGRATION.md operand-block example as a program) compiled with gcc; called by
    __graft_entry__.build(), run by tests/test_scale_gpu.py on the prebuilt kernel of FORMS[0]."""
    exe = c_host_path()
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.dirname(drs.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "native", "capi_ops_host.c"), "-o", exe, "-L", libdir, "-ldrstencil_amd", "-Wl,-rpath," + libdir,
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


# ---- emulated plugins (the CPU suite) -----------------------------------------------------------------------------------------------
def build_emulated(workdir, stc_path, options, read_log=False):
    """drstencil <options> -> emitted source -> host shared object (tests/emu), its entry points typed (Emulated).  read_log: compiled
    with tests/source_readlog.h in front, which exports drs_readlog_watch(base, bytes, map)."""
    from emu_util import CLANG, DRSTENCIL, EMU_INC, SUPPORT
    stc_dir, name = os.path.split(os.path.abspath(stc_path))
    tag = hashlib.md5((" ".join(options) + open(stc_path).read()).encode()).hexdigest()[:12]
    src = os.path.join(str(workdir), "k_%s.hip" % tag)
    so = os.path.join(str(workdir), "k_%s_emu%s.so" % (tag, "_log" if read_log else ""))
    p = subprocess.run([DRSTENCIL] + list(options) + ["-o", src, name], cwd=stc_dir, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and os.path.exists(src), (p.returncode, p.stdout)
    log = ["-include", os.path.join(ROOT, "tests", "source_readlog.h")] if read_log else []
    subprocess.check_call([CLANG, "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-DDRS_EMULATE", "-DDRS_PLUGIN",
                           "-I" + EMU_INC, "-I" + SUPPORT] + log + ["-x", "c++", src, "-o", so])
    lib = Emulated(so)
    if read_log:
        lib.lib.drs_readlog_watch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.lib.drs_readlog_watch.restype = None
    return lib


class Emulated:
    """An emulated plugin with one calling convention whatever its options: launch(in, out, F, res, X, W) -> 0, gold(in, out, F, X, W) -> 0
    on numpy arrays (F None without --source, res None without --residual, X None without --dirichlet, W None without --scale).  A --scale
    plugin exports drs_plugin_launch_ops and drs_plugin_launch_gold_ops and none of the other launch entry points."""
    OTHERS = dc.Emulated.OTHERS + ("drs_plugin_launch_fix", "drs_plugin_launch_gold_fix")

    def __init__(self, so):
        import json
        self.so = so
        self.lib = ctypes.CDLL(so)
        self.lib.drs_plugin_info.restype = ctypes.c_char_p
        self.info = json.loads(self.lib.drs_plugin_info().decode())
        self.scale = bool(self.info.get("scale"))
        self.dirichlet = bool(self.info.get("dirichlet"))
        self.source = bool(self.info.get("source"))
        self.residual_elems = int(self.info.get("residual_elems", 0))
        if self.scale:
            assert not any(hasattr(self.lib, n) for n in self.OTHERS)                # instead of, not beside
            self.lib.drs_plugin_launch_ops.argtypes = [ctypes.c_void_p] * 7
            self.lib.drs_plugin_launch_gold_ops.argtypes = [ctypes.c_void_p] * 6
            self.plain = None
        else:
            assert not hasattr(self.lib, "drs_plugin_launch_ops") and not hasattr(self.lib, "drs_plugin_launch_gold_ops")
            self.plain = dc.Emulated(so)

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def launch(self, a, b, F=None, res=None, X=None, W=None):
        assert (W is not None) == self.scale
        if not self.scale:
            return self.plain.launch(a, b, F, res, X)
        assert (F is not None) == self.source and (res is not None) == bool(self.residual_elems) and (X is not None) == self.dirichlet
        assert res is None or res.size == self.residual_elems
        return self.lib.drs_plugin_launch_ops(self._p(a), self._p(b), self._p(F), self._p(res), self._p(X), self._p(W), None)

    def gold(self, a, b, F=None, X=None, W=None):
        assert (W is not None) == self.scale
        if not self.scale:
            return self.plain.gold(a, b, F, X)
        return self.lib.drs_plugin_launch_gold_ops(self._p(a), self._p(b), self._p(F), self._p(X), self._p(W), None)


def load_emulated(so):
    return Emulated(so)
