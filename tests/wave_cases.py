"""Kernel configurations of the --time-order 2 tests (tests/test_time_order_cpu.py, tests/test_time_order_gpu.py) and of
scripts/wave_cost.py, prebuilt by __graft_entry__.build() so that the GPU box finds them in drstencil_amd/_kcache.  Also the host
reference the tests share: out = S(in) - out_old on the interior, as two correctly rounded operations (the oracle's contracted sweep,
then one subtraction in the array's dtype), so every comparison is bit for bit, in fp32 and fp64, for any number of launches."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STC = os.path.join(ROOT, "tests", "stc")
ORDER2 = ["--time-order", "2"]
PERIODIC = ["--boundary", "periodic"]


def stc(name):
    return os.path.join(STC, name + ".stc")


# (id, ndim, stc, options): one seeded case per step-1 schedule (scatter, reuse, window; taps and rows order; register and LDS-DMA staging;
# 2D tiles and streams) with the store-path knobs --store-mask buffer, --defer-stores and --zigzag in 3D.  Not here: strided merges,
# loader wavefronts, overlapped x rims, window loads and drains, unpacked rows, coefficients in registers, non-temporal accesses, XCD
# maps, rotation moduli, prefetch depths beyond 1 -- tests/test_mode_fuzz_cpu.py (explicit cases and a sample of the tuner's space) and
# tests/test_mode_fuzz_gpu.py cover those
SMALL = [
    ("3d_star_fp32", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--sn", "8"]),
    ("3d_star_oddN_fp64_elem", 3, stc("t3_star_odd"), ["--3d", "--dtype", "fp64"]),
    ("3d_cross_reuse_dist2", 3, stc("t3_cross"), ["--3d", "--dtype", "fp32", "--dist", "2"]),
    ("3d_window_prefetch", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--schedule", "window", "--prefetch", "--sn", "16"]),
    ("3d_rows_prefetch", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--order", "rows", "--prefetch", "--sn", "16"]),
    ("3d_dma_fp64", 3, stc("t3_star"), ["--3d", "--dtype", "fp64", "--stage", "dma", "--sn", "8"]),
    ("3d_store_mask_buffer", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--store-mask", "buffer", "--prefetch", "--sn", "8", "--by", "8", "--block-merge-y", "2"]),
    ("3d_defer_stores", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--defer-stores", "1", "--prefetch", "--sn", "8", "--by", "8", "--block-merge-y", "2"]),
    ("3d_zigzag", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--zigzag", "1", "--sn", "16"]),
    ("3d_ahead_fp64", 3, stc("t3_ahead"), ["--3d", "--dtype", "fp64", "--sn", "8", "--prefetch"]),
    ("2d_star_tile_fp32", 2, stc("t2_star"), ["--dtype", "fp32"]),
    ("2d_box25_tile_fp64", 2, stc("t2_box25"), ["--dtype", "fp64"]),
    ("2d_star_stream_fp32", 2, stc("t2_star"), ["--dtype", "fp32", "--streaming", "--sn", "40"]),
    ("2d_odd_stream_fp64", 2, stc("t2_odd"), ["--dtype", "fp64", "--streaming"]),
]
SMALL = [(c, n, s, o + ORDER2) for c, n, s, o in SMALL]

# periodic + order 2 against the host reference with wrap, and the analytic plane wave (fp64)
PERIODIC_CASE = ("3d_wave_periodic_fp32", 3, stc("t3_wave"), ["--3d", "--dtype", "fp32", "--sn", "8", "--prefetch"] + PERIODIC + ORDER2)
PLANE_WAVE = ("3d_plane_wave_fp64", 3, stc("t3_wave"), ["--3d", "--dtype", "fp64", "--sn", "8"] + PERIODIC + ORDER2)
# the emitted standalone program with --check
CHECK_PROGRAM = ("3d_wave_check_program", 3, stc("t3_wave"), ["--3d", "--dtype", "fp64", "--check"] + PERIODIC + ORDER2)
# guard-band arena checks: one 3D and one 2D case
ARENA = [SMALL[0], SMALL[10]]


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def step1_tuned(w):
    """The tuner's step-1 row of workload `w` (a bench.WORKLOADS key) as a full option list."""
    from drstencil_amd import tuned_defaults as td
    wl = _bench().WORKLOADS[w]
    return list(td.options_for(wl["stc"], wl["ndim"], wl["dtype"]))


def full_cases():
    """BASELINE sizes, one launch each: C4 1024^3 and C2 8192^2, fp32, the tuned step-1 row plus --time-order 2."""
    b = _bench()
    return [("C4_step1_order2", 3, b.WORKLOADS["c4"]["stc"], step1_tuned("c4") + ORDER2),
            ("C2_step1_order2", 2, b.WORKLOADS["c2"]["stc"], step1_tuned("c2") + ORDER2)]


def cost_cases():
    """scripts/wave_cost.py: (id, workload, step-1 options, the same with --time-order 2)."""
    return [(w, w, step1_tuned(w), step1_tuned(w) + ORDER2) for w in ("c4", "c2")]


def all_build_args():
    out = [c[3] + [c[2]] for c in SMALL + [PERIODIC_CASE, PLANE_WAVE] + full_cases()]
    b = _bench()
    for _, w, first, second in cost_cases():
        out += [first + [b.WORKLOADS[w]["stc"]], second + [b.WORKLOADS[w]["stc"]]]
    return out


def check_program_path():
    return os.path.join(ROOT, "drstencil_amd", "_kcache", "emitted_programs", "wave_check")


def build_check_program(drs):
    """Generate and compile the standalone --check --time-order 2 program (run by tests/test_time_order_gpu.py); called by
    __graft_entry__.build(), so that no test starts hipcc."""
    import shutil
    import subprocess
    exe = check_program_path()
    out = os.path.dirname(exe)
    os.makedirs(out, exist_ok=True)
    shutil.copy(os.path.join(drs.SUPPORT_DIR, "common.hpp"), out)
    _, _, src, opts = CHECK_PROGRAM
    # the kernel name is the .stc path minus 4 characters: run from the spec's directory
    subprocess.check_call([drs.CLI_PATH] + opts + ["-o", exe + ".hip", os.path.basename(src)], cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-o", exe, exe + ".hip"])
    return exe


# ---- host reference ---------------------------------------------------------------------------------------------------------------
def interior(a, H):
    return a[tuple(slice(H, n - H) for n in a.shape)]


def host_launch(spec, src, dst, periodic=False):
    """One --time-order 2 launch src -> dst in place: dst[interior] = S(src)[interior] - dst[interior].  The sweep is the oracle's fused
    FMA chain rounded once, the subtraction one more rounded operation in the array's dtype; dst's ring is left alone."""
    import oracle
    H = spec.halo
    if periodic:
        from periodic_cases import host_wrap
        host_wrap(src, H)
    tmp = dst.copy()
    oracle.sweep(spec, src, tmp, contract=1)
    d = interior(dst, H)
    d[...] = interior(tmp, H) - d
    return dst


def host_run(spec, A, B, launches, periodic=False):
    """`launches` launches of the ping-pong loop k(A,B); k(B,A); ... in place (an odd count ends on B)."""
    for t in range(launches):
        src, dst = (A, B) if t % 2 == 0 else (B, A)
        host_launch(spec, src, dst, periodic)
    return launches


# ---- the analytic plane wave (t3_wave, periodic): no oracle involved ----------------------------------------------------------------
def plane_wave(shape, H, points, m=(1, 2, 3)):
    """(A, B, exact): interior A = cos(k.x), B = cos(k.x + w) with k_d = 2 pi m_d / P_d over the period P = shape - 2 H and
    cos w = (c0 + 2 lambda sum cos k_d) / 2 for the star `points` (centre c0, neighbours lambda).  u(t) = cos(k.x - w t) solves
    u(t+1) = S(u(t)) - u(t-1) exactly; exact(n) is the interior of the array written by launch n (1-based) of the ping-pong from
    A = u(0), B = u(-1): u(n)."""
    c0 = dict(points)[(0, 0, 0)]
    lam = dict(points)[(0, 0, 1)]
    P = [n - 2 * H for n in shape]
    k = [2.0 * np.pi * md / pd for md, pd in zip(m, P)]
    w = np.arccos((c0 + 2.0 * lam * sum(np.cos(kd) for kd in k)) / 2.0)
    grids = np.meshgrid(*[np.arange(pd, dtype=np.float64) for pd in P], indexing="ij")
    phase = sum(kd * g for kd, g in zip(k, grids))
    A = np.zeros(shape, np.float64)
    B = np.zeros(shape, np.float64)
    interior(A, H)[...] = np.cos(phase)
    interior(B, H)[...] = np.cos(phase + w)
    return A, B, (lambda n: np.cos(phase - n * w))
