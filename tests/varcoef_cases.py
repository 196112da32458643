"""Kernel configurations of the --varcoef tests (tests/test_varcoef_cpu.py under the CPU emulation, tests/test_varcoef_gpu.py on the GPU:
the same list in both places) and of scripts/varcoef_cost.py, prebuilt by __graft_entry__.build() so that the GPU box finds them in
drstencil_amd/_kcache and no GPU test starts the compiler.  Also what the two suites share: the emulated plugin's loader, the inputs and
the host reference.

The reference of one launch (in -> out), host_launch, is independent of the generator's arithmetic text: the ring fill of the non-fixed
axes on `in`, then the gold-order chain over the taps t of oracle.Spec(...).points
    v = a_0[I] * in[I + d_0];   v = fma(a_t[I], in[I + d_t], v), t = 1 .. T-1
with libm's correctly rounded fmaf / fma over whole arrays (tests/native/fma_ref.c), then numpy operations in the array's dtype on the
interior I, one rounding each, in the contract's order -- tests/scale_cases.py's: w *, the centre term, - out_old, + src, the select,
the residual.

The coefficients: 1.5 * signed_random, seeded per tap -- both signs, magnitudes above 1, different in every cell and every tap, so that a
swapped pair of tap grids or a plane lead off by one cannot cancel.

The geometries are tests/residual_cases.py's (EDGE, BIG, its buffer-mask form, the step-1 KNOBS and MODES); the option refuses fused
steps, so those are left out, and it refuses packed pairs, so the rows-order geometry runs unpacked.  SMALLER lists the geometries that
spill with T coefficient values per point, cross-compiling for gfx950 (the runtime refuses a kernel that spills; that rule stays), with
the measured scratch; they run on tiles of fewer rows per lane.

The sample of the tuner's space (sample_jobs): fuzz_parity.make_jobs(20, seed, "order2") with --time-order 2 replaced by --varcoef.
SAMPLE_SEED is the first seed for which at most 5 of the 20 are refused, cross-compiling for gfx950; REFUSED lists them."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

import dirichlet_cases as dc
import residual_cases as rc
import scale_cases as sc
from residual_cases import F32, F64, ORDER2, RES, ROOT, SOURCE, dtype_of, interior, residual_of, same_bits, stc  # noqa: F401

VC = ["--varcoef"]
DIR = dc.DIR


def with_vc(opts):
    return list(opts) + VC


def plain_opts(opts):
    return [o for o in opts if o != "--varcoef"]


EDGE = dc.EDGE                      # min_333 periodic (one interior cell), thin 7x9x13 (branch, buffer, fp64), tile_plus1 (branch, buffer)
# Geometries that spill with T coefficient values per point, cross-compiling for gfx950, run on tiles of fewer rows per lane (the options
# are appended: the last value wins).  Most of them leave the rows per lane to the default, 8: 7 taps x 8 rows x 4 points are 224 registers
# in fp32.  Measured on the geometry as the other suites run it, bytes of scratch per lane (s: spilled scalar registers):
_Y2 = ["--by", "8", "--block-merge-y", "2"]
_Y1 = ["--by", "8", "--block-merge-y", "1"]
_W32 = ["--bx", "32", "--by", "8", "--block-merge-y", "1"]           # 256 lanes: a lane may have 512 registers
_HALF = ["--by", "4", "--block-merge-y", "2"]
SMALLER = {
    "star_70x45x530_early_exits": _HALF,                # 864; the 16 x 4 lanes stay: 64 x 8 tiles, 486 of 488 launched workgroups have a tile
    "star_70x45x530_early_exits_buffer": _HALF,         # 1088, 84 s
    "prefetch_depth2": _Y2,                             # 1288 (with --source --residual max: 2060)
    "cyclic_merge_x2_fp64": _Y2,                        # 1380
    "loader_waves_fp64": _Y2,                           # 1824
    "shape_11_3d_o2_fp32": _W32,                        # 22 taps: 616 at 64 x 4 lanes x 2 rows, 364 at 64 x 8 x 1 (512 lanes: 256 registers)
    "shape_05_3d_o2_fp64": _W32,                        # 56 taps: 96 at 64 x 8 lanes x 1 row
    "order2_fp32_varcoef": _Y2,                         # 1164
    "source_fp64_varcoef": _Y2,                         # 1344
    "order2_source_buffer_varcoef": _Y1,                # 8 s at 4 x 2 rows
    "reflect_fp32_varcoef": _Y2,                        # 916
    "channel_fp64_varcoef": _Y2,                        # 984
    "order2_fp32_all": _Y1,                             # 2544, 5 s; 160 at 8 x 2 rows
    "source_fp64_all": _Y2,                             # 2056
    "order2_source_buffer_all": _Y1,                    # 15 s at 4 x 2 rows
    "reflect_fp32_all": _Y2,                            # 1664, 8 s
    "channel_fp64_all": _Y2,                            # 2056
    "int_lap3_fp32": _Y2,                               # 1044
    "int_lap3_fp64_buffer": _Y2,                        # 1068, 38 s
    "int_shape11_fp32": _W32,                           # 436 at 4 x 2 rows, 308 at 8 x 1
}


def _fit(c):
    return (c[0], c[1], c[2], list(c[3]) + SMALLER.get(c[0], []))


def _unpacked(c):
    """The rows-order geometry without packed pairs (--varcoef refuses --pack 1)."""
    if c[0] != "rows_pack":
        return c
    o = list(c[3])
    o[o.index("--pack") + 1] = "0"
    return ("rows_unpacked", c[1], c[2], o)


BIG = _fit(dc.BIG)                  # 70 x 45 x 530 with early-leaving workgroups
BIG_BUFFER = _fit(dc.BIG_BUFFER)
KNOBS = [_fit(_unpacked(c)) for c in dc.KNOBS]
# a sum that starts late (every tap ahead along the streamed dimension), zh = 2 with five distinct leads, 25 taps in fp64
STENCILS = [_fit(c) for c in [
    ("ahead_3d_fp32", 3, stc("t3_ahead"), F32 + ["--sn", "8", "--prefetch"] + _HALF),
    ("ahead_3d_fp64_buffer", 3, stc("t3_ahead"), F64 + ["--sn", "8", "--store-mask", "buffer"] + _HALF),
    ("ahead_2d_stream_fp32", 2, stc("t2_ahead"), ["--dtype", "fp32", "--streaming", "--sn", "40", "--prefetch"]),
    ("ahead_2d_tile_fp64", 2, stc("t2_ahead"), ["--dtype", "fp64", "--by", "4", "--block-merge-y", "2"]),
    ("shape_11_3d_o2_fp32", 3, stc("shape_11_3d_o2"), F32 + ["--sn", "8", "--prefetch"]),
    ("shape_05_3d_o2_fp64", 3, stc("shape_05_3d_o2"), F64 + ["--sn", "8"]),
    ("box25_2d_fp64", 2, stc("t2_box25"), ["--dtype", "fp64", "--by", "8", "--block-merge-y", "1"]),
    ("box25_2d_stream_fp64", 2, stc("t2_box25"), ["--dtype", "fp64", "--streaming", "--sn", "32"]),
]]
GEOMS = EDGE + [BIG, BIG_BUFFER] + KNOBS + STENCILS
CASES = list(GEOMS)
# every mode with --varcoef alone, and with every other option at once (--scale --scale-centre 0.3 --time-order 2 --source --dirichlet
# --residual max, r after every launch)
_ALL_TAIL = sc.SCALE + ["--scale-centre", "0.3"]
MODES = [_fit((c[0] + "_varcoef", c[1], c[2], c[3])) for c in rc.MODES] + \
        [_fit((c[0] + "_all", c[1], c[2], sc._all_of(c[0], c[3]) + _ALL_TAIL)) for c in rc.MODES]
# constant arrays: the arrays of the same command without the option (plain kernels prebuilt too)
UNCHANGED = [EDGE[1], [c for c in KNOBS if c[0] == "store_mask_buffer"][0], KNOBS[0], [c for c in KNOBS if c[0] == "tile_2d_fp32"][0], STENCILS[0], STENCILS[6]]
# exact integers, tap identity, special values
LAP3, LAP2 = stc("lap3"), stc("lap2")
INTEGER = [_fit(c) for c in [("int_lap3_fp32", 3, LAP3, F32 + ["--sn", "8", "--prefetch"]), ("int_lap3_fp64_buffer", 3, LAP3, F64 + ["--sn", "8", "--store-mask", "buffer"]),
                             ("int_shape11_fp32", 3, stc("shape_11_3d_o2"), F32 + ["--sn", "8"])]]
# 3d7pt_star fp64 at 448^3: the last tap's grid starts past byte offset 2^32 (GPU only; tests/test_varcoef_gpu.py writes the spec)
INT_BIG_DIM = 448
INT_BIG_OPTS = F64 + ["--bx", "64", "--by", "4", "--block-merge-y", "2", "--sn", "8", "--prefetch"]
IDENTITY = [("identity_thin_fp32", 3, stc("edge3_thin"), EDGE[1][3]), ("identity_lap3_fp64", 3, LAP3, F64 + ["--sn", "8", "--prefetch"] + _HALF),
            ("identity_lap2_stream_fp32", 2, LAP2, ["--dtype", "fp32", "--streaming", "--sn", "16"])]
SPECIAL = [EDGE[4], EDGE[5]]            # N = 2 Halo + 257, branch and buffer masks: an x seam, eight corners
# the memory contract under PROT_NONE pages: the edge grids and three knob cases; the read log: no buffer masks (the emulated window load is
# a plain dereference)
CONTRACT = EDGE + [c for c in KNOBS if c[0] in ("prefetch_depth2", "store_mask_buffer", "stream_2d_fp32")]
READLOG = [EDGE[1], EDGE[4]] + [c for c in KNOBS if c[0] in ("odd_elem_fp64", "prefetch_depth2", "loader_waves_fp64", "stream_2d_dma_fp64", "tile_2d_fp32")] + [STENCILS[0]]
# (prefetch_depth2 with --source --residual max on top spills 92 bytes at 8 x 2 rows: one row per lane)
ARENA = [EDGE[5], (KNOBS[0][0], KNOBS[0][1], KNOBS[0][2], KNOBS[0][3] + _Y1), [c for c in KNOBS if c[0] == "tile_2d_fp32"][0]]
# run to tolerance: Jacobi for -div(kappa grad u) = f on lap3 / lap2 (the shape and the tap order; the values are not used)
SOLVE = [("divgrad_lap3_fp32", 3, LAP3, F32 + ["--sn", "8"] + _Y2, 1e-4), ("divgrad_lap3_fp64", 3, LAP3, F64 + ["--sn", "8"] + _Y2, 1e-9),
         ("divgrad_lap2_fp64", 2, LAP2, ["--dtype", "fp64"], 1e-9)]
SOLVE_DIMS = {3: (8, 8, 8), 2: (1, 12, 12)}
MAX_LAUNCHES = 4000
CHECK_PROGRAM = ("3d_varcoef_check_program", 3, LAP3, ["--3d", "--dtype", "fp64", "--check", "--boundary", "periodic"] + ORDER2 + SOURCE + VC)
BENCH_CONFIGS = ["c1_2d5pt_star_4096", "c2_2d5pt_star_8192", "c3_3d7pt_star_512", "c4_3d7pt_star_1024", "c5_2d25pt_box_16384"]


# ---- the correctly rounded fused multiply-add -------------------------------------------------------------------------------------------
def fma_lib_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "c_host", "libfma_ref.so")


def build_fma_lib():
    """tests/native/fma_ref.c compiled with gcc (no -mfma: every element is one call of libm's fmaf / fma); called by
    __graft_entry__.build(), and by the first CPU test that needs it where build() has not run."""
    so = fma_lib_path()
    os.makedirs(os.path.dirname(so), exist_ok=True)
    tmp = so + ".%d.tmp" % os.getpid()
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "fma_ref.c"), "-o", tmp, "-lm"])
    os.replace(tmp, so)
    return so


_FMA = None


def _fma_lib():
    global _FMA
    if _FMA is None:
        so = fma_lib_path()
        if not os.path.exists(so):
            build_fma_lib()
        _FMA = ctypes.CDLL(so)
        for n in ("vc_fmaf", "vc_fma"):
            getattr(_FMA, n).argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t]
            getattr(_FMA, n).restype = None
    return _FMA


def fma(a, b, c):
    """round(a * b + c) once, element by element, by libm."""
    dt = a.dtype
    assert dt == b.dtype == c.dtype and a.shape == b.shape == c.shape and dt in (np.float32, np.float64)
    a, b, c = (np.ascontiguousarray(x) for x in (a, b, c))
    out = np.empty(a.shape, dt)
    (_fma_lib().vc_fmaf if dt == np.float32 else _fma_lib().vc_fma)(a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data, a.size)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def taps_of(spec):
    """The taps in gold order as offsets in the array's own dimensions: (k, j, i) in 3D, (j, i) in 2D."""
    return [tuple(off[3 - len(spec.shape):]) for off, _ in spec.points]


def coefficients(spec, dt, seed=11):
    """(T,) + grid: 1.5 * signed_random, seeded per tap."""
    from fuzz_parity import signed_random
    return np.stack([(signed_random(spec.shape, dt, seed + 20 + t) * 1.5).astype(dt) for t in range(len(spec.points))])


def constant_coefficients(spec, dt):
    """a_t = (real_t)(c_t) everywhere, c_t as the emitted source writes it (six significant digits)."""
    K = np.empty((len(spec.points),) + tuple(spec.shape), dt)
    for t, (_, c) in enumerate(spec.points):
        K[t] = np.asarray(float("%g" % c), dt)
    return K


def inputs(spec, opts, seed=11):
    """(A, B, F or None, fix or None, w or None, coef)."""
    A, B, F, X, W = sc.inputs(spec, opts, seed)
    return A, B, F, X, (W if "--scale" in opts else None), coefficients(spec, dtype_of(opts), seed)


def _hash(shape):
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return ((idx * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0xFFFFFFFF)


def integer_problem(spec, dt, seed=5):
    """in in [-4, 4], a_t[p] = ((t * 7 + hash(p)) mod 7) - 3, hash taken of the element's index in the whole (T, grid) array (of the cell's
    index alone every tap's grid would be the same): every product and sum is exact.  (A, coef, want): want is the interior of one launch
    by plain integer numpy."""
    H = spec.halo
    shape = tuple(spec.shape)
    Ai = np.random.default_rng(seed).integers(-4, 5, shape).astype(np.int64)
    taps = taps_of(spec)
    h = _hash((len(taps),) + shape)
    Ki = np.stack([((np.uint64(t * 7) + h[t]) % np.uint64(7)).astype(np.int64) - 3 for t in range(len(taps))])
    want = np.zeros(interior(Ai, H).shape, np.int64)
    for t, d in enumerate(taps):
        want += interior(Ki[t], H) * Ai[tuple(slice(H + o, n - H + o) for o, n in zip(d, shape))]
    return Ai.astype(dt), Ki.astype(dt), want


def special_problem(spec, opts, info, held):
    """Coefficients holding +0.0, -0.0, +-inf, NaN and the smallest subnormals of either sign at corners and seams, a different tap's grid
    at each cell; +inf and -0.0 planted in `in` at two interior sites; with --dirichlet the inf site's neighbours are partly held."""
    A, B, F, X, W, K = inputs(spec, opts)
    dt = A.dtype
    sp = sc.w_specials(dt)
    for n, c in enumerate(rc.planted_cells(info)):
        K[n % len(K)][c] = sp[n % len(sp)]
    H = spec.halo
    mid = tuple((H + (d - H - 1)) // 2 for d in spec.shape)
    p = mid[:-1] + (mid[-1] - 6,)
    q = mid[:-1] + (mid[-1] + 6,)
    A[p] = np.inf
    A[tuple(slice(c - H, c + H + 1) for c in q)] = -0.0
    if held:
        X[p] = 0.5
        X[q] = np.asarray(np.nan, dt)
    return A, B, F, X, W, K, p, q


def identity_cells(info, shape):
    """Three interior cells of the tap-identity test: the first corner, a cell on a tile seam in x (the first column of the last tile; the
    last column where there is one tile) and on a stream-block seam where there is one, and a cell in the middle."""
    H, nd = info["halo"], len(shape)
    mid = tuple((H + (n - H - 1)) // 2 for n in shape)
    sx = H + info["tile_owned_cols"] * (info["tiles_x"] - 1) if info["tiles_x"] > 1 else shape[-1] - H - 1
    seam = list(mid[:-1]) + [sx]
    if info["streams"] and info["stream_blocks"] > 1:
        seam[0] = H + info["sn"] * (info["stream_blocks"] // 2)
    assert all(H <= c < n - H for c, n in zip(seam, shape))
    return [(H,) * nd, tuple(seam), tuple(m + 1 for m in mid)]


# ---- host reference ------------------------------------------------------------------------------------------------------------------
def chain(spec, src, K):
    """The gold-order chain on the interior: one rounded product, then one correctly rounded fma per tap."""
    H = spec.halo
    v = None
    with np.errstate(invalid="ignore", over="ignore"):
        for t, d in enumerate(taps_of(spec)):
            x = np.ascontiguousarray(src[tuple(slice(H + o, n - H + o) for o, n in zip(d, src.shape))])
            a = np.ascontiguousarray(interior(K[t], H))
            v = a * x if v is None else fma(a, x, v)
    assert v.dtype == src.dtype
    return v


def host_launch(spec, ndim, opts, src, dst, F, X, W, K):
    """One launch src -> dst of a kernel generated with `opts` (with --varcoef in them), in place.  Returns the residual of the stored
    arrays (a 0-d array of the dtype)."""
    import boundary_cases
    H = spec.halo
    modes = boundary_cases.modes_of(list(opts) + ["x"], ndim)
    if any(m != "fixed" for m in modes):
        boundary_cases.host_fill(src, H, modes)
    r = chain(spec, src, K)
    d = interior(dst, H)
    with np.errstate(invalid="ignore", over="ignore"):
        if "--scale" in opts:
            r = sc.scaled(r, interior(W, H), interior(src, H), np.asarray(sc.centre_of(opts), src.dtype)[()])
        if "--time-order" in opts:
            r = r - d
        if "--source" in opts:
            r = r + interior(F, H)
        if "--dirichlet" in opts:
            f = interior(X, H)
            r = np.where(np.isnan(f), r, f)
        assert r.dtype == src.dtype
        d[...] = r
        return residual_of(src, dst, H)


# ---- run to tolerance: Jacobi for -div(kappa grad u) = f ------------------------------------------------------------------------------
def divgrad_problem(spec, dt):
    """Two-valued kappa with a jump (1 and 10, the jump on a plane through the middle of the last axis), face coefficients by the harmonic
    mean, f = 1, a ring of 0.  Jacobi: u'[p] = sum_faces (k_face / diag[p]) u[p + d] + f / diag[p], diag = the sum of the six (four) face
    coefficients; the centre tap's coefficient is 0.  (A, B, src, coef), everything starting at 0."""
    shape = tuple(spec.shape)
    kappa = np.ones(shape, np.float64)
    kappa[..., shape[-1] // 2:] = 10.0
    taps = taps_of(spec)
    face = []
    for d in taps:
        if not any(d):
            face.append(None)
            continue
        nb = np.roll(kappa, tuple(-o for o in d), axis=tuple(range(len(shape))))       # kappa[p + d] (the wrapped ring is never used: its cells are not computed)
        face.append(2.0 * kappa * nb / (kappa + nb))
    diag = sum(f for f in face if f is not None)
    K = np.stack([np.zeros(shape) if f is None else f / diag for f in face]).astype(dt)
    F = np.zeros(shape, dt)
    interior(F, spec.halo)[...] = interior((1.0 / diag).astype(dt), spec.halo)
    A = np.zeros(shape, dt)
    return A, A.copy(), F, K


def oracle_solve(spec, ndim, A, B, F, K, tol, max_launches, check_every):
    """The run to tolerance as a numpy loop of the host reference that looks at r at the same launches: (status, launches, r)."""
    n, r = 0, None
    limit = max_launches - max_launches % 2
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            for src, dst in ((A, B), (B, A)):
                r = host_launch(spec, ndim, SOURCE + VC, src, dst, F, None, None, K)
                n += 1
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r


def solve_opts(opts):
    return with_vc(list(opts) + SOURCE + RES)


def solve_stc(workdir, ndim, src):
    """The stencil of `src` on the small grid of the run-to-tolerance cases."""
    from helpers import write_stc
    import oracle
    pts = [tuple(off[3 - ndim:]) + (c,) for off, c in oracle.Spec(src, ndim, 1).points]
    path = os.path.join(str(workdir), "divgrad%d.stc" % ndim)
    write_stc(path, ndim, SOLVE_DIMS[ndim], 4, pts)
    return path


# ---- the sample of the tuner's space ------------------------------------------------------------------------------------------------
SAMPLE_SEED = 1
SAMPLE_SIZE = 20
MIN_CHECKED = 15                                                  # at most 5 of 20 refused
# what build() refuses of the sample, cross-compiling for gfx950: (index in the sample, reason)
REFUSED = [(4, "spills 44 bytes per lane to scratch memory (448 lanes, element-wide rows)"), (5, "spills 48 bytes per lane to scratch memory (1024 lanes: 128 registers)"),
           (9, "--varcoef cannot be combined with --coef (the sample draws --coef vgpr)"), (12, "--stage dma needs 16-byte vectors: the 2D grid's rows are no multiple of 4 fp32"),
           (19, "--varcoef cannot be combined with --coef (the sample draws --coef sgpr)")]


def sample_jobs(seed=None):
    """fuzz_parity's tuples (ndim, stc, dtype, args, step) with --time-order 2 replaced by --varcoef."""
    import fuzz_parity
    out = []
    for ndim, path, dtype, args, step in fuzz_parity.make_jobs(SAMPLE_SIZE, SAMPLE_SEED if seed is None else seed, "order2"):
        a = list(args)
        i = a.index("--time-order")
        a[i:i + 2] = VC
        out.append((ndim, path, dtype, a, step))
    return out


# ---- what build() compiles -----------------------------------------------------------------------------------------------------------
def bare_args(w):
    """The bare --varcoef command on a bench.WORKLOADS configuration (the fit rule steps the tuned row down)."""
    wl = rc._bench().WORKLOADS[w]
    return (["--3d"] if wl["ndim"] == 3 else []) + ["--dtype", wl["dtype"]] + VC + [wl["stc"]]


def all_build_args():
    out = [with_vc(c[3]) + [c[2]] for c in CASES + MODES + INTEGER + IDENTITY]
    out += [with_vc(c[3]) + [c[2]] for c in UNCHANGED] + [list(c[3]) + [c[2]] for c in UNCHANGED]
    out += [with_vc(c[3]) + [c[2]] for c in SPECIAL] + [with_vc(c[3] + DIR) + [c[2]] for c in SPECIAL]
    out += [with_vc(c[3] + SOURCE + RES) + [c[2]] for c in ARENA]
    # the operand block on old kinds of kernel: plain, --source, --dirichlet, --residual, --scale
    out += [list(o) + [EDGE[1][2]] for o in (EDGE[1][3], EDGE[1][3] + SOURCE, EDGE[1][3] + DIR, EDGE[1][3] + RES, EDGE[1][3] + sc.SCALE)]
    seen, uniq = set(), []
    for a in out:
        if tuple(a) not in seen:
            seen.add(tuple(a))
            uniq.append(a)
    return uniq


def gpu_stc_dir():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "varcoef_stc")


def gpu_solve_stc(ndim, src):
    """The run-to-tolerance spec of the GPU suite (written by build(), read by the tests)."""
    os.makedirs(gpu_stc_dir(), exist_ok=True)
    return solve_stc(gpu_stc_dir(), ndim, src)


def int_big_stc():
    """3d7pt_star on INT_BIG_DIM^3 (written by build(), read by the GPU test)."""
    from helpers import write_stc
    import oracle
    os.makedirs(gpu_stc_dir(), exist_ok=True)
    path = os.path.join(gpu_stc_dir(), "star_%d.stc" % INT_BIG_DIM)
    pts = [tuple(off) + (c,) for off, c in oracle.Spec(os.path.join(ROOT, "benchmarks", "3d7pt_star", "3d7pt_star.stc"), 3, 1).points]
    write_stc(path, 3, (INT_BIG_DIM,) * 3, 4, pts)
    return path


def generated_build_args():
    """Kernels on specs that build() writes (the run-to-tolerance grids, the 448^3 star)."""
    out = [solve_opts(o) + [gpu_solve_stc(ndim, src)] for _, ndim, src, o, _ in SOLVE]
    out.append(with_vc(INT_BIG_OPTS) + [int_big_stc()])
    return out


def cost_cases():
    """scripts/varcoef_cost.py: (workload, the tuned step-1 options, the same at the stepped-down geometry, that with --varcoef).  The
    stepped-down geometry is read from the generator's note on the bare --varcoef command."""
    import re
    import source_cases
    import drstencil_amd as drs
    out = []
    for w in ("c2", "c4"):
        tuned = source_cases.step1_tuned(w)
        rc_, msg, _ = drs.generate(bare_args(w))
        m = re.search(r"stepped down to (.*)$", msg, re.M)
        geo = m.group(1).split() if m else []
        down = [o for n, o in enumerate(tuned) if not (o in geo[::2] or (n and tuned[n - 1] in geo[::2]))] + geo       # the row's own geometry words give way
        out.append((w, tuned, down, with_vc(down)))
    return out


def cost_build_args():
    b = rc._bench()
    out = []
    for w, tuned, down, vc in cost_cases():
        out += [o + [b.WORKLOADS[w]["stc"]] for o in (tuned, down, vc)]
    return out


def check_program_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "emitted_programs", "varcoef_check")


def build_check_program(drs):
    """Generate and compile the standalone --check --varcoef program (run by tests/test_varcoef_gpu.py); called by
    __graft_entry__.build(), so that no test starts hipcc."""
    import shutil
    exe = check_program_path()
    out = os.path.dirname(exe)
    os.makedirs(out, exist_ok=True)
    shutil.copy(os.path.join(drs.SUPPORT_DIR, "common.hpp"), out)
    _, _, src, opts = CHECK_PROGRAM
    subprocess.check_call([drs.CLI_PATH] + opts + ["-o", exe + ".hip", os.path.basename(src)], cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-o", exe, exe + ".hip"])
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
    """An emulated plugin with one calling convention whatever its options: launch(in, out, F, res, X, W, K) -> 0 and
    gold(in, out, F, X, W, K) -> 0 on numpy arrays (None where the kernel takes none).  A --varcoef plugin exports drs_plugin_launch_ops
    and drs_plugin_launch_gold_ops with one more pointer, and none of the other launch entry points."""

    def __init__(self, so):
        import json
        self.so = so
        self.lib = ctypes.CDLL(so)
        self.lib.drs_plugin_info.restype = ctypes.c_char_p
        self.info = json.loads(self.lib.drs_plugin_info().decode())
        self.varcoef = bool(self.info.get("varcoef"))
        self.scale = bool(self.info.get("scale"))
        self.dirichlet = bool(self.info.get("dirichlet"))
        self.source = bool(self.info.get("source"))
        self.residual_elems = int(self.info.get("residual_elems", 0))
        if self.varcoef:
            assert not any(hasattr(self.lib, n) for n in sc.Emulated.OTHERS)                # instead of, not beside
            self.lib.drs_plugin_launch_ops.argtypes = [ctypes.c_void_p] * 8
            self.lib.drs_plugin_launch_gold_ops.argtypes = [ctypes.c_void_p] * 7
            self.plain = None
        else:
            self.plain = sc.Emulated(so)

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def launch(self, a, b, F=None, res=None, X=None, W=None, K=None):
        assert (K is not None) == self.varcoef
        if not self.varcoef:
            return self.plain.launch(a, b, F, res, X, W)
        assert (F is not None) == self.source and (res is not None) == bool(self.residual_elems) and (X is not None) == self.dirichlet and (W is not None) == self.scale
        assert res is None or res.size == self.residual_elems
        assert K.flags.c_contiguous and K.shape == (self.info["taps"],) + a.shape and K.dtype == a.dtype
        return self.lib.drs_plugin_launch_ops(self._p(a), self._p(b), self._p(F), self._p(res), self._p(X), self._p(W), self._p(K), None)

    def gold(self, a, b, F=None, X=None, W=None, K=None):
        assert (K is not None) == self.varcoef
        if not self.varcoef:
            return self.plain.gold(a, b, F, X, W)
        return self.lib.drs_plugin_launch_gold_ops(self._p(a), self._p(b), self._p(F), self._p(X), self._p(W), self._p(K), None)


def load_emulated(so):
    return Emulated(so)
