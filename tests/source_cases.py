"""Kernel configurations of the --source tests (tests/test_source_cpu.py, tests/test_source_gpu.py) and of scripts/source_cost.py,
prebuilt by __graft_entry__.build() so that the GPU box finds them in drstencil_amd/_kcache and no GPU test starts the compiler.  Also
the host reference the tests share: out = S(in) + src on the interior (with --time-order 2: (S(in) - out_old) + src) as two or three
correctly rounded operations -- the oracle's contracted sweep, then numpy operations in the array's dtype -- with the host ring fill in
front where a boundary is not fixed, so every comparison is bit for bit, in fp32 and fp64, for any number of launches.

The samples of the tuner's space (sample_jobs): fuzz_parity.make_jobs(20, seed, "order2") with --time-order 2 replaced by --source
("source", seed 4), or kept with --source added ("order2_source", seed 5).  Refusals are decided when build() compiles (the runtime
refuses kernels that spill, the generator rejects an LDS demand beyond the limit or LDS-DMA staging on rows that are no multiple of the
16-byte vector), so they are known before any GPU run.  Cross-compiling for gfx950, build() printed for these samples:
    source fuzz source: 16 kernels built, 4 refused
    source fuzz order2_source: 18 kernels built, 2 refused
Both suites assert at least MIN_CHECKED of each sample checked."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STC = os.path.join(ROOT, "tests", "stc")
SOURCE = ["--source"]
ORDER2 = ["--time-order", "2"]
PERIODIC = ["--boundary", "periodic"]
CHANNEL = ["--boundary", "periodic", "--boundary-z", "reflect"]


def stc(name):
    return os.path.join(STC, name + ".stc")


def _plain(opts):
    """An option list of wave_cases without its --time-order 2."""
    o = list(opts)
    i = o.index("--time-order")
    del o[i:i + 2]
    return o


def _wave_small():
    import wave_cases
    return wave_cases.SMALL


# the 14 step-1 configurations of wave_cases.SMALL with --time-order 2 replaced by --source, and five of them with both options
SMALL = [(c, n, s, _plain(o) + SOURCE) for c, n, s, o in _wave_small()]
BOTH_IDS = ("3d_star_fp32", "3d_window_prefetch", "3d_dma_fp64", "3d_store_mask_buffer", "2d_star_stream_fp32")
BOTH = [(c + "_order2", n, s, _plain(o) + ORDER2 + SOURCE) for c, n, s, o in _wave_small() if c in BOTH_IDS]
# non-fixed boundaries: the ring fill touches `in` only
PERIODIC_CASE = ("3d_wave_periodic_fp32", 3, stc("t3_wave"), ["--3d", "--dtype", "fp32", "--sn", "8", "--prefetch"] + PERIODIC + SOURCE)
CHANNEL_CASE = ("3d_wave_channel_order2_fp64", 3, stc("t3_wave"), ["--3d", "--dtype", "fp64", "--sn", "8"] + CHANNEL + ORDER2 + SOURCE)
# the manufactured fixed point: F = u* - S(u*), one launch from u* returns u* (fp64, no oracle)
FIXED_POINT = ("3d_fixed_point_fp64", 3, stc("t3_star"), ["--3d", "--dtype", "fp64", "--sn", "8", "--prefetch"] + SOURCE)
# the emitted standalone program with --check
CHECK_PROGRAM = ("3d_source_check_program", 3, stc("t3_wave"), ["--3d", "--dtype", "fp64", "--check"] + PERIODIC + ORDER2 + SOURCE)
# guard-band arena checks: one 3D and one 2D case
ARENA = [SMALL[0], SMALL[10]]


def edge_cases():
    """(id, ndim, stc, options): the edge grids, each under the modest 16-lane geometry of mode_fuzz_cases._G3 and the default one."""
    import mode_fuzz_cases as m
    out = []
    for cid, name, opts in [
            ("min_333_fp32", "edge3_min_h1", ["--dtype", "fp32"]),                         # one interior cell; N * 4 % 16 != 0: element path
            ("min_333_fp32_periodic", "edge3_min_h1", ["--dtype", "fp32"] + PERIODIC),
            ("thin_7x9x13_fp32", "edge3_thin", ["--dtype", "fp32"]),
            ("thin_7x9x13_fp64", "edge3_thin", ["--dtype", "fp64"]),
            ("tile_plus1_fp32", "edge3_tile_plus1", ["--dtype", "fp32"]),                  # N = 2 Halo + 257: the last tile stores one column
            ("tile_plus1_fp32_buffer", "edge3_tile_plus1", ["--dtype", "fp32", "--store-mask", "buffer"])]:
        for gid, g in (("modest", m._G3), ("default", [])):
            out.append(("%s_%s" % (cid, gid), 3, stc(name), ["--3d"] + opts + g + SOURCE))
    return out


def modes_of(opts, ndim):
    import boundary_cases
    return boundary_cases.modes_of(opts, ndim)


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def step1_tuned(w):
    import wave_cases
    return wave_cases.step1_tuned(w)


def full_cases():
    """BASELINE sizes, one launch each: C4 1024^3 and C2 8192^2, fp32, the tuned step-1 row plus --source."""
    b = _bench()
    return [("C4_step1_source", 3, b.WORKLOADS["c4"]["stc"], step1_tuned("c4") + SOURCE),
            ("C2_step1_source", 2, b.WORKLOADS["c2"]["stc"], step1_tuned("c2") + SOURCE)]


def cost_cases():
    """scripts/source_cost.py: (workload, step-1 options, with --source, with --time-order 2 --source)."""
    return [(w, step1_tuned(w), step1_tuned(w) + SOURCE, step1_tuned(w) + ORDER2 + SOURCE) for w in ("c4", "c2")]


# ---- the samples of the tuner's space ---------------------------------------------------------------------------------------------
SAMPLES = {"source": 4, "order2_source": 5}     # sample -> seed of fuzz_parity.make_jobs(20, seed, "order2")
SAMPLE_SIZE = 20
MIN_CHECKED = 15                                # three quarters of a sample
# On the tiny grids of the emulated suite (tests/test_source_cpu.py: SMALL_GRID) the generator refuses exactly these members, (sample,
# index) -> its reason on stderr; it refuses each for the same reason without --source (a tile geometry of the tuner's space whose LDS
# demand passes the limit, whatever the kernel computes).  Every other member is accepted and checked; the test asserts both.
EMU_REFUSED = {("source", 10): "drstencil: tile needs more than 160 KiB of LDS",
               ("order2_source", 3): "drstencil: tile needs more than 160 KiB of LDS"}


def sample_jobs(which):
    """fuzz_parity's tuples (ndim, stc, dtype, args, step) of sample `which`."""
    import fuzz_parity
    out = []
    for ndim, path, dtype, args, step in fuzz_parity.make_jobs(SAMPLE_SIZE, SAMPLES[which], "order2"):
        a = list(args)
        i = a.index("--time-order")
        a[i:i + 2] = SOURCE if which == "source" else ORDER2 + SOURCE
        out.append((ndim, path, dtype, a, step))
    return out


def all_build_args():
    out = [c[3] + [c[2]] for c in SMALL + BOTH + [PERIODIC_CASE, CHANNEL_CASE, FIXED_POINT] + edge_cases() + full_cases()]
    b = _bench()
    for w, first, second, third in cost_cases():
        out += [o + [b.WORKLOADS[w]["stc"]] for o in (first, second, third)]
    return out


def check_program_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "emitted_programs", "source_check")


def build_check_program(drs):
    """Generate and compile the standalone --check --source program (run by tests/test_source_gpu.py); called by
    __graft_entry__.build(), so that no test starts hipcc."""
    import shutil
    exe = check_program_path()
    out = os.path.dirname(exe)
    os.makedirs(out, exist_ok=True)
    shutil.copy(os.path.join(drs.SUPPORT_DIR, "common.hpp"), out)
    _, _, src, opts = CHECK_PROGRAM
    # the kernel name is the .stc path minus 4 characters: run from the spec's directory
    subprocess.check_call([drs.CLI_PATH] + opts + ["-o", exe + ".hip", os.path.basename(src)], cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-o", exe, exe + ".hip"])
    return exe


# ---- emulated plugins (the CPU suite): a --source plugin exports the three-pointer entry points only ----------------------------------
def build_emulated(workdir, stc_path, options, read_log=False):
    """drstencil <options> -> emitted source -> host shared object (tests/emu).  Returns the ctypes library with drs_plugin_launch_src
    and drs_plugin_launch_gold_src typed; raises AssertionError with the generator's output when it rejects the options.  read_log:
    compile with tests/source_readlog.h in front, which exports drs_readlog_watch(base, bytes, map)."""
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
    lib = load_emulated(so)
    if read_log:
        lib.drs_readlog_watch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.drs_readlog_watch.restype = None
    return lib


def load_emulated(so):
    lib = ctypes.CDLL(so)
    for n in ("drs_plugin_launch_src", "drs_plugin_launch_gold_src"):
        getattr(lib, n).argtypes = [ctypes.c_void_p] * 4
    lib.drs_plugin_info.restype = ctypes.c_char_p
    assert not hasattr(lib, "drs_plugin_launch") and not hasattr(lib, "drs_plugin_launch_gold")      # instead of, not beside
    return lib


# ---- host reference ---------------------------------------------------------------------------------------------------------------
def interior(a, H):
    return a[tuple(slice(H, n - H) for n in a.shape)]


def host_launch(spec, src, dst, F, modes=None, order2=False):
    """One --source launch src -> dst in place: dst[interior] = S(src)[interior] + F[interior], or with order2
    (S(src)[interior] - dst[interior]) + F[interior].  The sweep is the oracle's fused FMA chain rounded once; every further operation
    is one rounded numpy operation in the array's dtype, in this order.  modes: the boundary mode per axis, outermost first -- src's
    ring is filled first on the non-fixed ones.  dst's ring and F are left alone."""
    import oracle
    H = spec.halo
    if modes and any(m != "fixed" for m in modes):
        from boundary_cases import host_fill
        host_fill(src, H, modes)
    tmp = dst.copy()
    oracle.sweep(spec, src, tmp, contract=1)
    t = interior(tmp, H)
    d = interior(dst, H)
    if order2:
        t = t - d
    d[...] = t + interior(F, H)
    assert d.dtype == src.dtype == F.dtype
    return dst


def host_run(spec, A, B, F, launches, modes=None, order2=False):
    """`launches` launches of the ping-pong loop k(A,B,F); k(B,A,F); ... in place (an odd count ends on B)."""
    for t in range(launches):
        src, dst = (A, B) if t % 2 == 0 else (B, A)
        host_launch(spec, src, dst, F, modes, order2)
    return launches


def signed_random(shape, dtype, seed):
    """Uniform in [-1, 1)."""
    return (np.random.default_rng(seed).random(shape) * 2.0 - 1.0).astype(dtype)


def fixed_point(spec):
    """(u*, F) in fp64: u* a product of cosines over the whole grid, F = u* - S(u*) on the interior by shifted slices over spec.points
    (0 in the ring), so that S(u*) + F = u* up to the roundings of one chain and one addition."""
    shape = spec.shape
    H = spec.halo
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    u = np.ones(shape, np.float64)
    for g, n, m in zip(grids, shape, (1.0, 2.0, 3.0)):
        u = u * np.cos(2.0 * np.pi * m * (g + 0.25) / n)
    S = np.zeros(tuple(n - 2 * H for n in shape), np.float64)
    for off, c, *_ in spec.points:
        off = tuple(off)[3 - len(shape):]
        S += c * u[tuple(slice(H + o, n - H + o) for o, n in zip(off, shape))]
    F = np.zeros(shape, np.float64)
    interior(F, H)[...] = interior(u, H) - S
    return u, F
