"""Kernel configurations of the --boundary periodic tests (tests/test_periodic_gpu.py) and of scripts/periodic_cost.py, prebuilt by
__graft_entry__.build() so that the GPU box finds them in drstencil_amd/_kcache.  Also the host-side periodic reference the tests
share: fill a ring from its interior, and runs of the CPU oracle with that wrap in front of every launch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STC = os.path.join(ROOT, "tests", "stc")
CFG = os.path.join(ROOT, "benchmarks", "configs")
PERIODIC = ["--boundary", "periodic"]


def stc(name):
    return os.path.join(STC, name + ".stc")


# (id, ndim, stc, options): seeded small cases over the sweep's knobs -- every kernel treats the ring as read-only input, so each of them
# computes the periodic answer once the ring holds the images of the interior
SMALL = [
    ("3d_s1_fp32", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--sn", "8"]),
    ("3d_s1_fp64_oddN", 3, stc("t3_star_odd"), ["--3d", "--dtype", "fp64"]),
    ("3d_fused2_fp32", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "16"]),
    ("3d_fused3_fp32", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--step", "3", "--sn", "16"]),
    ("3d_fused2_fp64", 3, stc("t3_star"), ["--3d", "--dtype", "fp64", "--step", "2", "--sn", "16"]),
    ("3d_odd_fp64_step2", 3, stc("t3_odd"), ["--3d", "--dtype", "fp64", "--step", "2"]),
    ("3d_cross_reuse_dist2", 3, stc("t3_cross"), ["--3d", "--dtype", "fp32", "--dist", "2"]),
    ("3d_window_fp32", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--step", "2", "--schedule", "window", "--sn", "16", "--prefetch"]),
    ("3d_rows_fp32", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "16", "--prefetch", "--order", "rows"]),
    ("3d_dma_fp64", 3, stc("t3_star"), ["--3d", "--dtype", "fp64", "--stage", "dma", "--sn", "8"]),
    ("3d_zigzag_fp32", 3, stc("t3_star"), ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "16", "--zigzag", "1"]),
    ("3d_t3_skew_fp64", 3, stc("t3_star"), ["--3d", "--dtype", "fp64", "--step", "3", "--temporal", "1", "--skew", "1", "--pin", "1", "--exact-y", "1",
                                            "--bx", "34", "--by", "8", "--block-merge-y", "2", "--sn", "16", "--xcd-remap", "4"]),
    ("3d_t4_force_fp64", 3, stc("t3_star"), ["--3d", "--dtype", "fp64", "--step", "4", "--temporal", "force", "--prefetch", "--prefetch-depth", "2",
                                             "--bx", "36", "--by", "11", "--block-merge-y", "2", "--sn", "16", "--xcd-remap", "4"]),
    ("2d_tile_fp32", 2, stc("t2_star"), ["--dtype", "fp32"]),
    ("2d_box25_tile_fp64", 2, stc("t2_box25"), ["--dtype", "fp64"]),
    ("2d_stream_fp32", 2, stc("t2_star"), ["--dtype", "fp32", "--streaming", "--sn", "40"]),
    ("2d_odd_stream_fp64_step2", 2, stc("t2_odd"), ["--dtype", "fp64", "--step", "2", "--streaming"]),
]
SMALL = [(c, n, s, o + PERIODIC) for c, n, s, o in SMALL]

# the np.roll semantics check: Kernel.run for the spec's iterations on a small 3D fp64 case
ROLL = ("3d_fused2_fp64_roll", 3, stc("t3_star"), ["--3d", "--dtype", "fp64", "--step", "2", "--sn", "16"] + PERIODIC)


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def full_cases():
    """BASELINE sizes, periodic: C4 with the tuned headline options, C2 with its tuned tile."""
    b = _bench()
    return [("C4_headline_periodic", 3, b.WORKLOADS["c4"]["stc"], list(b.TUNED["c4"]) + PERIODIC),
            ("C2_tile_periodic", 2, b.WORKLOADS["c2"]["stc"], list(b.TUNED["c2"]) + PERIODIC)]


def cost_cases():
    """scripts/periodic_cost.py: (id, workload, fixed options, periodic options)."""
    b = _bench()
    out = []
    for cid, w, opts in (("c4", "c4", b.TUNED["c4"]), ("c2", "c2", b.TUNED["c2"]), ("c4f64_temporal4", "c4f64", b.TEMPORAL4["c4f64"])):
        out.append((cid, w, list(opts), list(opts) + PERIODIC))
    return out


def all_build_args():
    out = [c[3] + [c[2]] for c in SMALL] + [ROLL[3] + [ROLL[2]]] + [c[3] + [c[2]] for c in full_cases()]
    b = _bench()
    out += [per + [b.WORKLOADS[w]["stc"]] for _, w, _, per in cost_cases()]
    return out


# ---- host reference ---------------------------------------------------------------------------------------------------------------
def host_wrap(a, H):
    """Fill a's ring of width H from its interior, in place: the ghost at x takes x + P (x < H) or x - P (x >= n - H), P = n - 2H, each
    axis on its own (axis by axis over the full extent of the others, so edges and corners come out right).  Equals
    np.pad(interior, H, mode="wrap") without a second array."""
    for ax in range(a.ndim):
        n = a.shape[ax]
        P = n - 2 * H
        assert P >= H, "period shorter than the ring"

        def sl(s):
            return tuple(s if d == ax else slice(None) for d in range(a.ndim))
        a[sl(slice(0, H))] = a[sl(slice(P, P + H))]
        a[sl(slice(n - H, n))] = a[sl(slice(H, 2 * H))]
    return a


def oracle_periodic_run(spec, A, B, launches=None):
    """The ping-pong loop with the wrap in front of every launch, in place (A, B as the kernel's run() leaves them)."""
    import oracle
    n = spec.launches if launches is None else launches
    H = spec.halo
    for t in range(n):
        src, dst = (A, B) if t % 2 == 0 else (B, A)
        host_wrap(src, H)
        oracle.sweep(spec, src, dst, contract=1)
    return n


def roll_reference(points, interior, steps):
    """`steps` periodic updates of the one-step stencil over the period in float64 with np.roll (no oracle involved).
    points: [((k, j, i), coef)] of the one-step stencil; interior: the periodic domain (2D arrays take (j, i) offsets)."""
    u = np.asarray(interior, dtype=np.float64)
    for _ in range(steps):
        v = np.zeros_like(u)
        for off, c in points:
            d = off if u.ndim == 3 else off[1:]
            v += c * np.roll(u, tuple(-x for x in d), axis=tuple(range(u.ndim)))
        u = v
    return u
