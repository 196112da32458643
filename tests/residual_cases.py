"""Kernel configurations of the --residual tests (tests/test_residual_cpu.py under the CPU emulation, tests/test_residual_gpu.py on the
GPU: the same list in both places) and of scripts/residual_cost.py, prebuilt by __graft_entry__.build() so that the GPU box finds them in
drstencil_amd/_kcache and no GPU test starts the compiler.  Also what the two suites share: the emulated plugin's loader, the host
reference and the planted cells.

The reference of one launch (in -> out): the arrays by the job's existing host reference (tests/options_reference.py), then
    r = np.max(np.abs(out[I] - in[I]))
on the interior I in the array's dtype -- one rounded subtraction, the sign cleared, numpy's maximum, which propagates NaN.  A maximum
is the same in every order, so the kernel's value equals it in bits on every schedule, or both are NaN.

The sample of the tuner's space (sample_jobs): fuzz_parity.make_jobs(20, seed, "order2") -- step 1, no on-chip stages, which the
option refuses (half of a sample with them was refused for that alone; fused steps are in CASES) -- with --time-order 2 replaced by
--residual max.  Refusals are decided when build() compiles (the generator refuses an LDS demand beyond the limit and LDS-DMA staging
on rows that are no multiple of the 16-byte vector; the runtime refuses kernels that spill), so they are known before any GPU run.  SAMPLE_SEED is the first seed for which at most a quarter of the 20 is refused,
cross-compiling for gfx950."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STC = os.path.join(ROOT, "tests", "stc")
RES = ["--residual", "max"]
SOURCE = ["--source"]
ORDER2 = ["--time-order", "2"]
_G3 = ["--bx", "16", "--by", "4", "--block-merge-y", "2", "--sn", "4"]      # mode_fuzz_cases' modest geometry
_W256 = ["--bx", "64", "--by", "4", "--block-merge-x", "4", "--block-merge-y", "2", "--sn", "4"]     # 256 columns per tile: 4 points per lane


def stc(name):
    return os.path.join(STC, name + ".stc")


F32, F64 = ["--3d", "--dtype", "fp32"], ["--3d", "--dtype", "fp64"]
# (id, ndim, spec, options without --residual)
EDGE = [
    ("min_333_fp32_periodic", 3, stc("edge3_min_h1"), F32 + ["--boundary", "periodic"]),           # one interior cell
    ("thin_7x9x13_fp32", 3, stc("edge3_thin"), F32 + _G3),
    ("thin_7x9x13_fp32_buffer", 3, stc("edge3_thin"), F32 + _G3 + ["--store-mask", "buffer"]),
    ("thin_7x9x13_fp64", 3, stc("edge3_thin"), F64),
    ("tile_plus1_fp32", 3, stc("edge3_tile_plus1"), F32 + _W256),                                  # N = 2 Halo + 257: the last tile owns one column
    ("tile_plus1_fp32_buffer", 3, stc("edge3_tile_plus1"), F32 + _W256 + ["--store-mask", "buffer"]),
    ("min_12x12_fp32_s4", 2, stc("edge2_min_h4"), ["--dtype", "fp32", "--step", "4"]),
]
# 70 x 45 x 530: 9 stream blocks of 8 planes, 18 tiles of 64 x 4 points, 168 launched workgroups for 162 tiles: some leave at once
BIG = ("star_70x45x530_early_exits", 3, stc("t3_star"), F32 + ["--bx", "16", "--by", "4", "--sn", "8"])
KNOBS = [
    ("prefetch_depth2", 3, stc("t3_star"), F32 + ["--sn", "8", "--prefetch", "--prefetch-depth", "2"]),
    ("defer_stores", 3, stc("t3_star"), F32 + ["--defer-stores", "1", "--prefetch", "--sn", "8", "--by", "8", "--block-merge-y", "2"]),
    ("rows_pack", 3, stc("t3_star"), F32 + ["--order", "rows", "--pack", "1", "--prefetch", "--sn", "16"]),
    ("cyclic_merge_x2_fp64", 3, stc("t3_star"), F64 + ["--cyclic-merge-x", "2", "--sn", "8"]),
    ("loader_waves_fp64", 3, stc("t3_star"), F64 + ["--stage", "dma", "--loader-waves", "1", "--sn", "8"]),
    ("store_mask_buffer", 3, stc("t3_star"), F32 + ["--store-mask", "buffer", "--prefetch", "--sn", "8", "--by", "8", "--block-merge-y", "2"]),
    ("tile_2d_fp32", 2, stc("t2_star"), ["--dtype", "fp32"]),
    ("tile_2d_box9_fp64", 2, stc("t2_box9"), ["--dtype", "fp64"]),
    ("stream_2d_fp32", 2, stc("t2_star"), ["--dtype", "fp32", "--streaming", "--sn", "40"]),
    ("stream_2d_dma_fp64", 2, stc("t2_box9"), ["--dtype", "fp64", "--streaming", "--stage", "dma"]),
    ("fused_step2_fp32", 3, stc("t3_star"), F32 + ["--step", "2", "--sn", "16", "--prefetch-depth", "1"]),      # (the automatic depth 3 spills with the centre sets)
    ("fused_step3_fp64", 3, stc("t3_star"), F64 + ["--step", "3", "--sn", "8"]),
    ("odd_elem_fp64", 3, stc("t3_star_odd"), F64),
]
MODES = [
    ("order2_fp32", 3, stc("t3_wave"), F32 + ["--sn", "8", "--prefetch"] + ORDER2),
    ("source_fp64", 3, stc("t3_wave"), F64 + ["--sn", "8"] + SOURCE),
    ("order2_source_buffer", 3, stc("t3_wave"), F32 + ["--sn", "8", "--prefetch", "--store-mask", "buffer", "--by", "4", "--block-merge-y", "2"] + ORDER2 + SOURCE),
    ("reflect_fp32", 3, stc("t3_wave"), F32 + ["--sn", "8", "--boundary", "reflect"]),
    ("channel_fp64", 3, stc("t3_wave"), F64 + ["--sn", "8", "--boundary", "periodic", "--boundary-z", "reflect", "--boundary-x", "fixed"]),
]
CASES = EDGE + [BIG] + KNOBS + MODES
# the planted maximum and the special values run on these two
PLANT = [BIG, EDGE[4]]
# arrays with and without the option, bit for bit
UNCHANGED = [EDGE[1], BIG, KNOBS[0], KNOBS[6], MODES[2]]
# the memory contract under PROT_NONE pages: the edge grids and four knob cases
CONTRACT = EDGE + [KNOBS[0], KNOBS[5], KNOBS[8], MODES[2]]
# guard-band arena on the GPU
ARENA = [EDGE[5], KNOBS[0], KNOBS[6]]
# run to tolerance
JACOBI3 = stc("jacobi3")
# (a stencil without a centre tap has no pair of taps one plane apart: the reuse partition needs --dist 2, as the reference's would)
SOLVE = [("jacobi3_fp32", 3, JACOBI3, F32 + ["--dist", "2", "--sn", "8"], 1e-4), ("jacobi3_fp64", 3, JACOBI3, F64 + ["--dist", "2", "--sn", "8"], 1e-9)]
POISSON2 = ("poisson2_12x12_fp64", 2, stc("poisson2"), ["--dtype", "fp64", "--dist", "2"] + SOURCE, 1e-9)
DIVERGE = ("t3_star_overflow_fp32", 3, stc("t3_star"), F32 + ["--sn", "8"])          # coefficients sum to 1.5: finfo.max overflows at once
SOLVE_DIMS = {"emu": (10, 10, 10), "gpu": (18, 18, 18)}
MAX_LAUNCHES = 4000
CHECK_PROGRAM = ("3d_residual_check_program", 3, stc("t3_wave"), ["--3d", "--dtype", "fp64", "--check", "--boundary", "periodic"] + ORDER2 + SOURCE + RES)


def with_res(opts):
    return list(opts) + RES


# ---- the sample of the tuner's space ------------------------------------------------------------------------------------------------
SAMPLE_SIZE = 20
SAMPLE_SEED = 1
MIN_CHECKED = 15                                # three quarters of the sample


def sample_jobs(seed=None):
    """fuzz_parity's tuples (ndim, stc, dtype, args, step) with --time-order 2 replaced by --residual max."""
    import fuzz_parity
    out = []
    for ndim, path, dtype, args, step in fuzz_parity.make_jobs(SAMPLE_SIZE, SAMPLE_SEED if seed is None else seed, "order2"):
        a = list(args)
        i = a.index("--time-order")
        a[i:i + 2] = RES
        out.append((ndim, path, dtype, a, step))
    return out


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def cost_cases():
    """scripts/residual_cost.py: (row, workload, plain options, the same with --residual)."""
    import wave_cases
    b = _bench()
    rows = [("C2 step 1", "c2", wave_cases.step1_tuned("c2")), ("C4 step 1", "c4", wave_cases.step1_tuned("c4"))]
    return [(r, w, o, with_res(o)) for r, w, o in rows] + [("C4 fused step 2", "c4", ["--3d", "--dtype", "fp32", "--step", "2"], ["--3d", "--dtype", "fp32", "--step", "2"] + RES)]


def solve_stc(workdir, which, ndim, src):
    """The spec of a run-to-tolerance case: tests/stc/jacobi3.stc is the GPU's 18^3 grid, the emulated suite runs its stencil on 10^3; the
    2D Poisson case keeps its own 12 x 12."""
    from helpers import write_stc
    import oracle
    if ndim == 2 or which == "gpu":
        return src
    pts = [tuple(off) + (c,) for off, c in oracle.Spec(src, 3, 1).points]
    path = os.path.join(str(workdir), "jacobi3_%d.stc" % SOLVE_DIMS[which][0])
    write_stc(path, 3, SOLVE_DIMS[which], 4, pts)
    return path


def all_build_args():
    out = []
    for c in CASES + [DIVERGE]:
        out.append(with_res(c[3]) + [c[2]])
    for c in UNCHANGED:
        out.append(list(c[3]) + [c[2]])
    for cid, ndim, src, opts, tol in SOLVE:
        out.append(with_res(opts) + [src])
    out.append(with_res(POISSON2[3]) + [POISSON2[2]])
    return out


def cost_build_args():
    b = _bench()
    out = []
    for row, w, plain, res in cost_cases():
        out += [plain + [b.WORKLOADS[w]["stc"]], res + [b.WORKLOADS[w]["stc"]]]
    return out


def check_program_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "emitted_programs", "residual_check")


def build_check_program(drs):
    """Generate and compile the standalone --check --residual program (run by tests/test_residual_gpu.py); called by
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
def build_emulated(workdir, stc_path, options):
    """drstencil <options> -> emitted source -> host shared object (tests/emu), its entry points typed (load_emulated)."""
    from emu_util import CLANG, DRSTENCIL, EMU_INC, SUPPORT
    stc_dir, name = os.path.split(os.path.abspath(stc_path))
    tag = hashlib.md5((" ".join(options) + open(stc_path).read()).encode()).hexdigest()[:12]
    src = os.path.join(str(workdir), "k_%s.hip" % tag)
    so = os.path.join(str(workdir), "k_%s_emu.so" % tag)
    p = subprocess.run([DRSTENCIL] + list(options) + ["-o", src, name], cwd=stc_dir, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and os.path.exists(src), (p.returncode, p.stdout)
    subprocess.check_call([CLANG, "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-DDRS_EMULATE", "-DDRS_PLUGIN",
                           "-I" + EMU_INC, "-I" + SUPPORT, "-x", "c++", src, "-o", so])
    return load_emulated(so)


class Emulated:
    """An emulated plugin with one calling convention whatever its options: launch(in, out, F, res) -> 0, gold(in, out, F) -> 0 on numpy
    arrays (F None without --source, res None without --residual)."""

    def __init__(self, so):
        import json
        self.lib = ctypes.CDLL(so)
        self.so = so
        self.lib.drs_plugin_info.restype = ctypes.c_char_p
        self.info = json.loads(self.lib.drs_plugin_info().decode())
        self.source = bool(self.info.get("source"))
        self.residual_elems = int(self.info.get("residual_elems", 0))
        vp = ctypes.c_void_p
        if self.residual_elems:
            assert not hasattr(self.lib, "drs_plugin_launch") and not hasattr(self.lib, "drs_plugin_launch_src")      # instead of, not beside
            self.lib.drs_plugin_launch_res.argtypes = [vp] * 5
        g = self.lib.drs_plugin_launch_gold_src if self.source else self.lib.drs_plugin_launch_gold
        g.argtypes = [vp] * (4 if self.source else 3)
        if not self.residual_elems:
            f = self.lib.drs_plugin_launch_src if self.source else self.lib.drs_plugin_launch
            f.argtypes = [vp] * (4 if self.source else 3)

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def launch(self, a, b, F=None, res=None):
        assert (F is not None) == self.source and (res is not None) == bool(self.residual_elems)
        if self.residual_elems:
            assert res.size == self.residual_elems
            return self.lib.drs_plugin_launch_res(self._p(a), self._p(b), self._p(F), self._p(res), None)
        if self.source:
            return self.lib.drs_plugin_launch_src(self._p(a), self._p(b), self._p(F), None)
        return self.lib.drs_plugin_launch(self._p(a), self._p(b), None)

    def gold(self, a, b, F=None):
        if self.source:
            return self.lib.drs_plugin_launch_gold_src(self._p(a), self._p(b), self._p(F), None)
        return self.lib.drs_plugin_launch_gold(self._p(a), self._p(b), None)


def load_emulated(so):
    return Emulated(so)


# ---- host reference -----------------------------------------------------------------------------------------------------------------
def interior(a, H):
    return a[tuple(slice(H, n - H) for n in a.shape)]


def step_of(opts):
    return int(opts[opts.index("--step") + 1]) if "--step" in opts else 1


def dtype_of(opts):
    return np.float32 if "fp32" in opts else np.float64


def residual_of(src, dst, H):
    """np.max(np.abs(out[I] - in[I])) in the array's dtype, as a 0-d array of that dtype."""
    d = np.abs(interior(dst, H) - interior(src, H))
    assert d.dtype == src.dtype
    with np.errstate(invalid="ignore"):
        return np.max(d)


def host_launch(spec, ndim, opts, src, dst, F):
    """One launch src -> dst of a kernel generated with `opts`, in place, by the job's existing reference, and its residual."""
    from options_reference import options_reference
    with np.errstate(invalid="ignore", over="ignore"):
        options_reference(spec, ndim, [o for o in opts if o not in RES], src, dst, F, 1)
        return residual_of(src, dst, spec.halo)


def same_bits(a, b):
    """Equal in bits, or both NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype, (a.dtype, b.dtype)
    return bool((np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes())


def inputs(spec, opts, seed=11):
    from fuzz_parity import signed_random
    dt = dtype_of(opts)
    F = signed_random(spec.shape, dt, seed + 2) if "--source" in opts else None
    return signed_random(spec.shape, dt, seed), signed_random(spec.shape, dt, seed + 1), F


def planted_cells(info):
    """Interior cells at which a planted value must be seen by exactly one lane of one workgroup: the eight interior corners and the two
    cells either side of a tile seam in x, in y and of a stream-block seam in z (where the kernel has such a seam)."""
    H = info["halo"]
    dims = (info["L"], info["M"], info["N"])
    lo, hi = [H] * 3, [d - H - 1 for d in dims]
    cells = [(z, y, x) for z in (lo[0], hi[0]) for y in (lo[1], hi[1]) for x in (lo[2], hi[2])]
    mid = [(a + b) // 2 for a, b in zip(lo, hi)]
    seams = []
    if info["tiles_x"] > 1:
        sx = H + info["tile_owned_cols"] * (info["tiles_x"] - 1)        # first column of the last tile
        seams += [(mid[0], mid[1], sx - 1), (mid[0], mid[1], sx)]
    if info["tiles_y"] > 1:
        sy = H + info["tile_owned_rows"] * (info["tiles_y"] // 2)
        seams += [(mid[0], sy - 1, mid[2]), (mid[0], sy, mid[2])]
    if info["stream_blocks"] > 1:
        sz = H + info["sn"] * (info["stream_blocks"] // 2)
        seams += [(sz - 1, mid[1], mid[2]), (sz, mid[1], mid[2])]
    for c in seams:
        assert all(l <= v <= h for v, l, h in zip(c, lo, hi)), (c, lo, hi)
    return cells + seams


def poisoned_input(A, spec):
    """A with NaN in every cell that neither a tap nor the centre stream reads: footprint.read_mask extended by the interior."""
    from footprint import interior_slices, nan_value, read_mask
    m = read_mask(spec)
    m[interior_slices(spec.shape, spec.halo)] = True
    P = A.copy()
    P[~m] = nan_value(P.dtype)
    return P


def oracle_solve(spec, A, B, F, tol, max_launches, check_every):
    """The run to tolerance as a numpy loop of oracle sweeps (contract=1) that looks at r at the same launches: (status, launches, r)."""
    import oracle
    H = spec.halo
    n, r = 0, None
    limit = max_launches - max_launches % 2
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            for src, dst in ((A, B), (B, A)):
                oracle.sweep(spec, src, dst, contract=1)
                if F is not None:
                    interior(dst, H)[...] = interior(dst, H) + interior(F, H)
                n += 1
        r = residual_of(B, A, H)               # the last launch was (B -> A)
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r
