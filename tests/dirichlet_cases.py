"""Kernel configurations of the --dirichlet tests (tests/test_dirichlet_cpu.py under the CPU emulation, tests/test_dirichlet_gpu.py on the
GPU: the same list in both places) and of scripts/dirichlet_cost.py, prebuilt by __graft_entry__.build() so that the GPU box finds them in
drstencil_amd/_kcache and no GPU test starts the compiler.  Also what the two suites share: the emulated plugin's loader, the seeded
pattern of held cells, the special-value construction and the host reference.

The geometries are tests/residual_cases.py's (EDGE, BIG and the step-1 KNOBS); the option refuses fused steps, so those are left out.

The reference of one launch (in -> out): the arrays by the job's existing host reference WITHOUT the option (tests/options_reference.py),
then on the interior I
    out[I] = np.where(np.isnan(fix[I]), out[I], fix[I])
which is a select: nothing is computed from a held value or from the value it replaces.  With --residual max the residual is then numpy's
max(abs(out[I] - in[I])) of the arrays as they stand.

The samples of the tuner's space (sample_jobs): fuzz_parity.make_jobs(20, seed, "order2") with --time-order 2 replaced by --dirichlet, and
make_jobs(20, seed, "order2_source") with --dirichlet appended.  Refusals are decided when build() compiles (the generator refuses an LDS
demand beyond the limit and LDS-DMA staging on rows that are no multiple of the 16-byte vector; the runtime refuses kernels that spill),
so they are known before any GPU run.  Each seed is the first for which at most a quarter of the 20 is refused, cross-compiling for gfx950."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

import residual_cases as rc
from residual_cases import F32, F64, ORDER2, RES, ROOT, SOURCE, dtype_of, interior, residual_of, same_bits, stc  # noqa: F401

DIR = ["--dirichlet"]

EDGE = [c for c in rc.EDGE if "--step" not in c[3]]                     # min_333 periodic, thin (branch, buffer, fp64), tile_plus1 (branch, buffer)
BIG = rc.BIG                                                            # 70 x 45 x 530 with early-exit workgroups
BIG_BUFFER = (BIG[0] + "_buffer", BIG[1], BIG[2], BIG[3] + ["--store-mask", "buffer"])
# 2D tile, 2D stream, DMA stream, buffer mask, deferred stores, rows + pack, cyclic merge, loader waves, depth 2, odd rows.  The fp64
# loader-wave kernel fills the register file at its default 64-column tile already (--source alone spills there too, and the runtime
# refuses a kernel that spills): with a third array it runs on 32-column tiles
KNOBS = [(c[0], c[1], c[2], c[3] + (["--bx", "32"] if c[0] == "loader_waves_fp64" else [])) for c in rc.KNOBS if "--step" not in c[3]]
MODES = list(rc.MODES) + [("residual_fp32", 3, stc("t3_wave"), F32 + ["--sn", "8", "--prefetch"] + RES)]
CASES = EDGE + [BIG, BIG_BUFFER] + KNOBS + MODES
MIN_333 = EDGE[0]
# every mode with --residual max as well: r after every launch
# (all five streams on the buffer-mask path at prefetch distance spill two scalar registers: that one loads its streams in the plane's own iteration)
RES_MODES = [(c + "_residual", n, s, [x for x in o if x != "--prefetch" or c != "order2_source_buffer"] + RES) for c, n, s, o in rc.MODES] + [MODES[-1]]
# planted cells and special values: BIG and tile_plus1, with branch and with buffer masks
PLANT = [BIG, BIG_BUFFER, EDGE[4], EDGE[5]]
# all free: the arrays of the same command without the option (plain kernels prebuilt too)
UNCHANGED = list(rc.UNCHANGED)
# the memory contract under PROT_NONE pages: the edge grids and four knob cases
CONTRACT = EDGE + [c for c in KNOBS if c[0] in ("prefetch_depth2", "store_mask_buffer", "stream_2d_fp32")] + [rc.MODES[2]]
# the read log over fix: 16-byte rows with partial vectors, element rows, prefetched and DMA-staged streams, the 2D tile, order 2 + source
READLOG = [EDGE[4], BIG] + [c for c in KNOBS if c[0] in ("odd_elem_fp64", "prefetch_depth2", "loader_waves_fp64", "stream_2d_dma_fp64", "tile_2d_fp32")] + \
          [("order2_source_fp32", 3, stc("t3_wave"), F32 + ["--sn", "8", "--prefetch"] + ORDER2 + SOURCE)]
# guard-band arena on the GPU
ARENA = [EDGE[5], KNOBS[0], [c for c in KNOBS if c[0] == "tile_2d_fp32"][0]]
# run to tolerance: residual_cases.SOLVE's kernels, tolerances and MAX_LAUNCHES with held cells
SOLVE = rc.SOLVE
SOLVE_DIMS = rc.SOLVE_DIMS
MAX_LAUNCHES = rc.MAX_LAUNCHES
SOLVE_KINDS = ("block", "lshape")
CHECK_PROGRAM = ("3d_dirichlet_check_program", 3, stc("t3_wave"), ["--3d", "--dtype", "fp64", "--check", "--boundary", "periodic"] + ORDER2 + SOURCE + RES + DIR)


def with_fix(opts):
    return list(opts) + DIR


# ---- the pattern of held cells ---------------------------------------------------------------------------------------------------------
def fix_pattern(shape, dtype, seed=17):
    """fix over the whole array: held with probability 1/4 at values in [-1, 1), free (NaN) elsewhere.  The ring gets the same treatment:
    no launch reads it."""
    r = np.random.default_rng(seed)
    held = r.random(shape) < 0.25
    vals = (r.random(shape) * 2.0 - 1.0).astype(dtype)
    return np.where(held, vals, np.asarray(np.nan, dtype)).astype(dtype)


def inputs(spec, opts, seed=11):
    """(A, B, F or None, fix)."""
    A, B, F = rc.inputs(spec, opts, seed)
    return A, B, F, fix_pattern(spec.shape, dtype_of(opts), seed + 6)


def held_and_free(X, H):
    """(held, free) interior cell counts of a fix array."""
    n = np.isnan(interior(X, H))
    return int((~n).sum()), int(n.sum())


_UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
# NaNs that mark free cells: both signs, quiet and signalling, nonzero payloads
FREE_NANS = {np.dtype(np.float32): [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FC0DEAD, 0xFFA5A5A5, 0x7FBFFFFF, 0xFFFFFFFF],
             np.dtype(np.float64): [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FF8DEAD0000BEEF,
                                    0xFFF5A5A5A5A5A5A5, 0x7FF7FFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF]}


def held_specials(dtype):
    """Held values that arithmetic would not keep: +0.0, -0.0, the smallest subnormal (either sign), +inf, -inf."""
    tiny = np.nextafter(np.asarray(0, dtype), np.asarray(1, dtype))
    return np.array([0.0, -0.0, tiny, -tiny, np.inf, -np.inf], dtype)


def special_problem(spec, opts, seed=11):
    """(A, B, F, fix, cells) for the special-value test.  fix: the seeded pattern with its free cells marked by every NaN of FREE_NANS in
    turn and every third held cell given one of held_specials in turn.  Four interior sites, far apart, are then BUILT:
      held_nan : in[p] = NaN and p held           -> the unheld value at p is NaN
      free_nan : the x neighbour of that p, free  -> its value is NaN
      held_inf : in[q] = +inf and q held (every coefficient of these stencils is positive and the centre tap exists) -> unheld +inf
      free_m0  : in = -0.0 on the whole neighbourhood of s (src there -0.0 too), s free -> S(in)[s] = -0.0
    Whether each site is what it is meant to be is asserted by the tests on the reference alone."""
    A, B, F, X = inputs(spec, opts, seed)
    dt = np.dtype(dtype_of(opts))
    H = spec.halo
    xi = interior(X, H)
    free = np.isnan(xi)
    bits = xi.view(_UINT[dt])
    nans = np.array(FREE_NANS[dt], _UINT[dt])
    bits[free] = nans[np.arange(int(free.sum())) % len(nans)]
    held_idx = np.argwhere(~free)[::3]
    sp = held_specials(dt)
    for n, c in enumerate(held_idx):
        xi[tuple(c)] = sp[n % len(sp)]
    dims = spec.shape
    lo = [H + 1] * 3
    hi = [d - H - 2 for d in dims]
    mid = [(a + b) // 2 for a, b in zip(lo, hi)]
    # three sites along x in the middle plane and row (x is the long axis of both grids)
    xs = [lo[2] + 3, mid[2], hi[2] - 3]
    p, q, s = [(mid[0], mid[1], x) for x in xs]
    pn = (p[0], p[1], p[2] + 1)
    nanq = np.asarray(np.nan, dt)
    A[p] = np.nan
    X[p] = 0.5
    X[pn] = nanq
    A[q] = np.inf
    X[q] = -0.25
    blk = tuple(slice(c - H, c + H + 1) for c in s)
    A[blk] = -0.0
    if F is not None:
        F[blk] = -0.0
    if "--time-order" in opts:
        B[s] = 0.0                   # -0.0 - (+0.0) = -0.0
    X[s] = nanq
    return A, B, F, X, {"held_nan": p, "free_nan": pn, "held_inf": q, "free_m0": s}


# ---- host reference -----------------------------------------------------------------------------------------------------------------
def plain_opts(opts):
    return [o for o in opts if o not in DIR]


def host_launch(spec, ndim, opts, src, dst, F, X, unheld=None):
    """One launch src -> dst of a kernel generated with `opts` (with or without --dirichlet in them) and held cells X, in place: the
    job's existing host reference without the option, then the select on the interior.  Returns the residual of the stored arrays (a
    0-d array of the dtype).  unheld: an array that receives the interior as it was in front of the select."""
    H = spec.halo
    rc.host_launch(spec, ndim, plain_opts(opts), src, dst, F)
    I, f = interior(dst, H), interior(X, H)
    if unheld is not None:
        interior(unheld, H)[...] = I
    I[...] = np.where(np.isnan(f), I, f)
    with np.errstate(invalid="ignore"):
        return residual_of(src, dst, H)


def oracle_solve(spec, A, B, F, X, tol, max_launches, check_every):
    """residual_cases.oracle_solve with the np.where after every sweep: (status, launches, r)."""
    import oracle
    H = spec.halo
    n, r = 0, None
    limit = max_launches - max_launches % 2
    f = interior(X, H)
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            for src, dst in ((A, B), (B, A)):
                oracle.sweep(spec, src, dst, contract=1)
                I = interior(dst, H)
                if F is not None:
                    I[...] = I + interior(F, H)
                I[...] = np.where(np.isnan(f), I, f)
                n += 1
        r = residual_of(B, A, H)               # the last launch was (B -> A)
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r


def solve_problem(spec, dt, kind):
    """(A, B, fix) of a run to tolerance on a cube with a ring of 0.  "block": everything starts at 0 and an inner block is held at 1.0
    (an electrode); "lshape": a random interior in [0, 1) and one octant held at 0, which leaves an L-shaped domain.  The held values are
    written into A and B, so every launch sees them."""
    H = spec.halo
    n = spec.shape[0]
    X = np.full(spec.shape, np.nan, dt)
    A = np.zeros(spec.shape, dt)
    if kind == "block":
        a, b = n // 2 - n // 8 - 1, n // 2 + n // 8 + 1
        X[a:b, a:b, a:b] = 1.0
    else:
        interior(A, H)[...] = np.random.default_rng(21).random(tuple(m - 2 * H for m in spec.shape)).astype(dt)
        X[H:n // 2, H:n // 2, H:n // 2] = 0.0
    held = ~np.isnan(X)
    A[held] = X[held]
    return A, A.copy(), X


# ---- the samples of the tuner's space --------------------------------------------------------------------------------------------------
SAMPLES = {"dirichlet": 1, "order2_source_dirichlet": 1}          # sample -> seed of fuzz_parity.make_jobs
SAMPLE_SIZE = 20
MIN_CHECKED = 15                                                  # three quarters of a sample


def sample_jobs(which, seed=None):
    """fuzz_parity's tuples (ndim, stc, dtype, args, step) of sample `which`."""
    import fuzz_parity
    seed = SAMPLES[which] if seed is None else seed
    out = []
    if which == "dirichlet":
        for ndim, path, dtype, args, step in fuzz_parity.make_jobs(SAMPLE_SIZE, seed, "order2"):
            a = list(args)
            i = a.index("--time-order")
            a[i:i + 2] = DIR
            out.append((ndim, path, dtype, a, step))
    else:
        for ndim, path, dtype, args, step in fuzz_parity.make_jobs(SAMPLE_SIZE, seed, "order2_source"):
            out.append((ndim, path, dtype, list(args[:-1]) + DIR + [args[-1]], step))
    return out


# ---- what build() compiles -----------------------------------------------------------------------------------------------------------
def cost_cases():
    """scripts/dirichlet_cost.py: (workload, tuned step-1 options, with --source, with --dirichlet)."""
    import source_cases
    return [(w, source_cases.step1_tuned(w), source_cases.step1_tuned(w) + SOURCE, source_cases.step1_tuned(w) + DIR) for w in ("c2", "c4")]


def all_build_args():
    out = [with_fix(c[3]) + [c[2]] for c in CASES + RES_MODES[:-1]]
    out += [list(c[3]) + [c[2]] for c in UNCHANGED]
    out += [with_fix(opts + RES) + [src] for cid, ndim, src, opts, tol in SOLVE]
    return out


def cost_build_args():
    b = rc._bench()
    out = []
    for w, plain, src, fix in cost_cases():
        out += [o + [b.WORKLOADS[w]["stc"]] for o in (plain, src, fix)]
    return out


def check_program_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "emitted_programs", "dirichlet_check")


def build_check_program(drs):
    """Generate and compile the standalone --check --dirichlet program (run by tests/test_dirichlet_gpu.py); called by
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
    """An emulated plugin with one calling convention whatever its options: launch(in, out, F, res, X) -> 0, gold(in, out, F, X) -> 0 on
    numpy arrays (F None without --source, res None without --residual, X None without --dirichlet).  A --dirichlet plugin exports
    drs_plugin_launch_fix and drs_plugin_launch_gold_fix and none of the other launch entry points."""
    OTHERS = ("drs_plugin_launch", "drs_plugin_launch_gold", "drs_plugin_launch_src", "drs_plugin_launch_gold_src", "drs_plugin_launch_res")

    def __init__(self, so):
        import json
        self.so = so
        self.lib = ctypes.CDLL(so)
        self.lib.drs_plugin_info.restype = ctypes.c_char_p
        self.info = json.loads(self.lib.drs_plugin_info().decode())
        self.dirichlet = bool(self.info.get("dirichlet"))
        self.source = bool(self.info.get("source"))
        self.residual_elems = int(self.info.get("residual_elems", 0))
        if self.dirichlet:
            assert not any(hasattr(self.lib, n) for n in self.OTHERS)                # instead of, not beside
            self.lib.drs_plugin_launch_fix.argtypes = [ctypes.c_void_p] * 6
            self.lib.drs_plugin_launch_gold_fix.argtypes = [ctypes.c_void_p] * 5
            self.plain = None
        else:
            assert not hasattr(self.lib, "drs_plugin_launch_fix") and not hasattr(self.lib, "drs_plugin_launch_gold_fix")
            self.plain = rc.Emulated(so)

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def launch(self, a, b, F=None, res=None, X=None):
        assert (X is not None) == self.dirichlet
        if not self.dirichlet:
            return self.plain.launch(a, b, F, res)
        assert (F is not None) == self.source and (res is not None) == bool(self.residual_elems)
        assert res is None or res.size == self.residual_elems
        return self.lib.drs_plugin_launch_fix(self._p(a), self._p(b), self._p(F), self._p(res), self._p(X), None)

    def gold(self, a, b, F=None, X=None):
        assert (X is not None) == self.dirichlet
        if not self.dirichlet:
            return self.plain.gold(a, b, F)
        return self.lib.drs_plugin_launch_gold_fix(self._p(a), self._p(b), self._p(F), self._p(X), None)


def load_emulated(so):
    return Emulated(so)
