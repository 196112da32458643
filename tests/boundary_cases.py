"""Kernel configurations of the reflecting / per-axis boundary tests (tests/test_boundary_axes_cpu.py, tests/test_boundary_axes_gpu.py)
and of scripts/periodic_cost.py --boundary reflect, prebuilt by __graft_entry__.build() so that the GPU box finds them in
drstencil_amd/_kcache and no GPU test starts the compiler.  Also the host reference the tests share: host_fill, the ring fill axis by
axis, and oracle_boundary_run, the CPU oracle with that fill in front of every launch.

The sample of the tuner's space (sample_jobs): 20 configurations of fuzz_parity.make_jobs(28, 4, "fixed") -- the fixed sweep gives
max(1, n // 14) jobs per spec and dtype, so n = 20 yields 14 and n = 28 is the smallest that yields 20 or more -- picked by a seeded
generator, each with a seeded per-axis mode triple appended (at least one non-fixed axis; axes shorter than 3 * Halo stay fixed).
Refusals are decided when build() compiles (the runtime refuses kernels that spill, the generator rejects an LDS demand beyond the limit
or LDS-DMA staging on rows that are no multiple of the 16-byte vector), so they are known before any GPU run.  Cross-compiling for gfx950,
build() printed for this sample:
    boundary fuzz: 17 kernels built, 3 refused
(all three for register spills), and of the 20 emulated on tiny grids by the CPU suite the generator
rejects none.  Both tests assert at least MIN_CHECKED checked."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STC = os.path.join(ROOT, "tests", "stc")
MODES = ("fixed", "periodic", "reflect")
REFLECT = ["--boundary", "reflect"]
MIXED3 = ["--boundary-z", "fixed", "--boundary-y", "periodic", "--boundary-x", "reflect"]
MIXED2 = ["--boundary-y", "periodic", "--boundary-x", "reflect"]
WALLS_X_FIXED = ["--boundary", "reflect", "--boundary-x", "fixed"]
ORDER2 = ["--time-order", "2"]


def stc(name):
    return os.path.join(STC, name + ".stc")


def settings(ndim):
    """The three boundary settings every whole-run case takes: (tag, options)."""
    return [("reflect", REFLECT), ("mixed", MIXED3 if ndim == 3 else MIXED2), ("reflect_xfixed", WALLS_X_FIXED)]


def modes_of(opts, ndim):
    """The per-axis modes an option list names, outermost axis first (the last value wins; a per-axis option overrides --boundary)."""
    given = {}
    for i, a in enumerate(opts[:-1]):
        if a in ("--boundary", "--boundary-z", "--boundary-y", "--boundary-x"):
            given[a] = opts[i + 1]
    axes = ("--boundary-z", "--boundary-y", "--boundary-x")[3 - ndim:]
    return tuple(given.get(a, given.get("--boundary", "fixed")) for a in axes)


def _base_small():
    import periodic_cases
    return [(c, n, s, o[:-2]) for c, n, s, o in periodic_cases.SMALL]        # the option lists without their --boundary periodic


def small_cases():
    """periodic_cases.SMALL with --boundary periodic replaced by each of the three settings: (id, ndim, stc, options)."""
    return [("%s_%s" % (c, tag), n, s, o + b) for c, n, s, o in _base_small() for tag, b in settings(n)]


# the GPU suite's part of them: the reflect and the mixed variant of five
GPU_SMALL_IDS = ("3d_fused2_fp32", "3d_rows_fp32", "3d_dma_fp64", "3d_t3_skew_fp64", "2d_stream_fp32")


def gpu_small_cases():
    return [("%s_%s" % (c, tag), n, s, o + b) for c, n, s, o in _base_small() if c in GPU_SMALL_IDS for tag, b in settings(n)[:2]]


def wave_cases_reflect():
    """The step-1 configurations of wave_cases.SMALL (--time-order 2) in a box with rigid walls."""
    import wave_cases
    return [(c + "_reflect", n, s, o + REFLECT) for c, n, s, o in wave_cases.SMALL]


# ---- edge grids (the specs and the two geometries of mode_fuzz_cases): (id, ndim, stc, options) ------------------------------------
def edge_cases():
    import mode_fuzz_cases as m
    out = []

    def add(cid, ndim, name, opts, geos):
        for gid, g in geos:
            out.append(("%s_%s" % (cid, gid), ndim, stc(name), (["--3d"] if ndim == 3 else []) + opts + g))
    g3 = [("modest", m._G3), ("default", [])]
    g2 = [("modest", m._G2), ("default", [])]
    add("min_333_fp32_reflect", 3, "edge3_min_h1", ["--dtype", "fp32"] + REFLECT, g3)                # one interior cell, every ghost its copy; element path
    add("min_666_fp64_s2_reflect", 3, "edge3_min_h2", ["--dtype", "fp64", "--step", "2"] + REFLECT, g3)
    add("min_666_fp64_s2_zper_yref_xfix", 3, "edge3_min_h2", ["--dtype", "fp64", "--step", "2", "--boundary-z", "periodic", "--boundary-y", "reflect"], g3)
    add("min_12x12_fp32_s4_reflect", 2, "edge2_min_h4", ["--dtype", "fp32", "--step", "4"] + REFLECT, g2)
    add("thin_7x9x13_fp32_s2_mixed", 3, "edge3_thin", ["--dtype", "fp32", "--step", "2"] + MIXED3, g3)
    add("thin_7x9x13_fp64_s2_mixed", 3, "edge3_thin", ["--dtype", "fp64", "--step", "2"] + MIXED3, g3)
    add("min_333_fp32_order2_reflect", 3, "edge3_min_h1", ["--dtype", "fp32"] + ORDER2 + REFLECT, g3)
    add("min_333_fp64_order2_reflect", 3, "edge3_min_h1", ["--dtype", "fp64"] + ORDER2 + REFLECT, g3)
    return out


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def full_case():
    """C4 1024^3 with the tuned headline options and rigid walls."""
    b = _bench()
    return ("C4_headline_reflect", 3, b.WORKLOADS["c4"]["stc"], list(b.TUNED["c4"]) + REFLECT)


def cost_cases(boundary="reflect"):
    """scripts/periodic_cost.py --boundary <mode>: (id, workload, fixed options, options with --boundary <mode>), C4 headline and C2 tile."""
    b = _bench()
    return [(cid, w, list(b.TUNED[w]), list(b.TUNED[w]) + ["--boundary", boundary]) for cid, w in (("c4", "c4"), ("c2", "c2"))]


# ---- the sample of the tuner's space ------------------------------------------------------------------------------------------------
SAMPLE = (20, 28, 4)        # (jobs, n of make_jobs, seed)
MIN_CHECKED = 15


def mode_triple(rnd, ndim, carries):
    """Per-axis options for a seeded triple with at least one non-fixed axis; `carries`[axis] false: that axis stays fixed."""
    while True:
        m = [rnd.choice(MODES) if ok else "fixed" for ok in carries]
        if any(x != "fixed" for x in m) or not any(carries):
            break
    opts = []
    for ax, v in zip(("--boundary-z", "--boundary-y", "--boundary-x")[3 - ndim:], m):
        opts += [ax, v]
    return opts


def sample_jobs(shape_of=None):
    """The 20 jobs as fuzz_parity's tuples (ndim, stc, dtype, args, step), the mode triple in front of the .stc.  shape_of(job) ->
    the grid the job will run on (default: its own spec's)."""
    import fuzz_parity
    import oracle
    jobs = fuzz_parity.make_jobs(SAMPLE[1], SAMPLE[2], "fixed")
    rnd = random.Random("boundary/%d" % SAMPLE[2])
    picked = sorted(rnd.sample(range(len(jobs)), SAMPLE[0]))
    out = []
    for n in picked:
        ndim, path, dtype, args, step = jobs[n]
        spec = oracle.Spec(path, ndim, step)
        shape = shape_of(jobs[n]) if shape_of else spec.shape
        carries = [d >= 3 * spec.halo for d in shape]
        out.append((ndim, path, dtype, args[:-1] + mode_triple(rnd, ndim, carries) + [path], step))
    return out


def all_build_args():
    out = [c[3] + [c[2]] for c in gpu_small_cases() + edge_cases() + [full_case()]]
    b = _bench()
    out += [opts + [b.WORKLOADS[w]["stc"]] for _, w, _, opts in cost_cases()]
    return out


# ---- host reference ---------------------------------------------------------------------------------------------------------------
def host_fill(a, H, modes):
    """Fill a's ring of width H on its non-fixed axes from its interior, in place: modes[axis] is "fixed" | "periodic" | "reflect",
    outermost axis first.  Axis by axis over the full extent of the other axes, fixed axes skipped: a cell with a coordinate in the ring
    of a non-fixed axis ends up with the value of the cell that has every coordinate mapped on its own (periodic: c + P below H, c - P
    from n - H on, P = n - 2H; reflect: 2H - 1 - c and 2(n - H) - 1 - c), and no other cell is written.  All-reflect equals
    np.pad(interior, H, mode="symmetric"), all-periodic np.pad(interior, H, mode="wrap")."""
    assert len(modes) == a.ndim, (modes, a.shape)
    for ax, mode in enumerate(modes):
        assert mode in MODES, mode
        if mode == "fixed":
            continue
        n = a.shape[ax]
        assert n >= 3 * H, "the interior of axis %d is shorter than the ring" % ax

        def sl(s):
            return tuple(s if d == ax else slice(None) for d in range(a.ndim))
        if mode == "periodic":
            a[sl(slice(0, H))] = a[sl(slice(n - 2 * H, n - H))]
            a[sl(slice(n - H, n))] = a[sl(slice(H, 2 * H))]
        else:
            a[sl(slice(0, H))] = a[sl(slice(2 * H - 1, H - 1, -1))]
            a[sl(slice(n - H, n))] = a[sl(slice(n - H - 1, n - 2 * H - 1, -1))]
    return a


def fill_destinations(shape, H, modes):
    """Boolean array: the cells host_fill writes (a coordinate in the ring of a non-fixed axis)."""
    m = np.zeros(shape, bool)
    for ax, mode in enumerate(modes):
        if mode != "fixed":
            idx = [slice(None)] * len(shape)
            for s in (slice(0, H), slice(shape[ax] - H, shape[ax])):
                idx[ax] = s
                m[tuple(idx)] = True
    return m


def oracle_boundary_run(spec, A, B, modes, launches=None, order2=False):
    """The ping-pong loop with host_fill in front of every launch, in place (A, B as the kernel's run() leaves them).  order2: each
    launch is out = S(in) - out_old on the interior (wave_cases.host_launch's two rounded operations)."""
    import oracle
    n = spec.launches if launches is None else launches
    H = spec.halo
    for t in range(n):
        src, dst = (A, B) if t % 2 == 0 else (B, A)
        host_fill(src, H, modes)
        if order2:
            import wave_cases
            wave_cases.host_launch(spec, src, dst)
        else:
            oracle.sweep(spec, src, dst, contract=1)
    return n
