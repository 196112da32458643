#!/usr/bin/env python3
"""emit_corpus.py OUTDIR [--lib libdrstencil_amd.so] [--cli drstencil] -- what the generator emits, pinned byte for byte.

For every argument list of the corpus one file OUTDIR/<nnnn>.txt: the list, the exit code, the messages (stdout + notes, as
drs_generate returns them), for a rejected list what the command prints on stderr, and the emitted source.  OUTDIR/MANIFEST has one
line per list: sha256 of that file, its number, the list.  Two generators emit the same text for the whole corpus iff `diff -r` of
their OUTDIRs is empty.  Nothing is compiled and no GPU is needed.

--lib / --cli name the generator under test (default: this tree's); the argument lists, and so the spec paths in the banners, always
come from THIS tree, so whole files compare equal.  To compare with another commit:

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/drstencil_amd/csrc
    scripts/emit_corpus.py /tmp/a --lib /tmp/parent/drstencil_amd/libdrstencil_amd.so --cli /tmp/parent/bin/drstencil
    scripts/emit_corpus.py /tmp/b && diff -r /tmp/a /tmp/b

The corpus: everything __graft_entry__.build() emits without a slab-view spec written into the cache; a seeded sample of the tuner's
r3 and r4 spaces; the host-program variants; one list per value of every option that selects an emitter
branch; the nine launch interfaces with and without --check in 2D and 3D, and the rows of the refusal table for --gpus N > 1 and
--pair-launch 1.  --coverage prints, per such option value, how many lists of the corpus carry it, and the lists per interface and row.
"""
import argparse
import ctypes
import hashlib
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STC = os.path.join(ROOT, "tests", "stc")


def stc(name):
    return os.path.join(STC, name + ".stc")


def build_lists():
    """The argument lists __graft_entry__.build() hands to the generator (those that need no spec written into the cache), as
    (cwd or None, list)."""
    from gpu_cases import all_build_args, golden_args, fuzz_sample_jobs
    from helpers import golden_cases, load_golden
    import bench
    import periodic_cases
    import wave_cases
    jobs = all_build_args()
    for c in golden_cases():
        meta = load_golden(c)[0]
        for rows in (False, True):
            opts, path = golden_args(c, meta, rows=rows)
            jobs.append(opts + [path])
    jobs += bench.kernel_arg_sets() + periodic_cases.all_build_args() + wave_cases.all_build_args()
    jobs += [j[3] for j in fuzz_sample_jobs()]
    for xrim in ("lds", "dpp"):
        jobs.append(["--dtype", "fp32", "--streaming", "--xrim", xrim, stc("t2_box25")])
    out = [(None, j) for j in jobs]
    # the standalone programs: generated from the spec's directory (the kernel name is the path minus ".stc")
    import conftest
    for name, opts in conftest.EMITTED_PROGRAMS.values():
        out.append((STC, list(opts) + [name + ".stc"]))
    _, _, src, opts = wave_cases.CHECK_PROGRAM
    out.append((os.path.dirname(src), list(opts) + [os.path.basename(src)]))
    # the six configurations of the tuner smoke run (same space, seed and order as build())
    from drstencil_amd.tuner import tuning as t
    t.order, t.ndim, t.elem_bytes = 1, 3, 4
    paras = t.enumerate_space((1, 2))
    random.seed(3)
    random.shuffle(paras)
    out += [(None, ["--3d", "--dtype", "fp32"] + t.cfgToCommandLine(v).split() + [stc("t3_star")]) for v in paras[:6]]
    return out


def space_sample(per=104, seed=11):
    """`per` configurations of each of (r3, r4) x (fp32, fp64) on t3_star, steps 1-3, every emission (the space's own filter
    leaves few for the generator to reject; those pin its error paths)."""
    from drstencil_amd.tuner import tuning as t
    out = []
    for r4 in (False, True):
        for dtype, eb in (("fp32", 4), ("fp64", 8)):
            t.order, t.ndim, t.elem_bytes = 1, 3, eb
            space = t.enumerate_space((1, 2, 3), emits=("taps", "pin", "rows", "rowspk"), round4=r4)
            rnd = random.Random("%d/%s/%d" % (seed, dtype, r4))
            for v in rnd.sample(space, per):
                out.append((None, ["--3d", "--dtype", dtype] + t.cfgToCommandLine(v).split() + [stc("t3_star")]))
    return out


# option values that select an emitter branch: (words on the command line, the bases they are tried on)
D3 = ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "16", "--prefetch"]
D3F64 = ["--3d", "--dtype", "fp64", "--sn", "8"]
PIPE = ["--3d", "--dtype", "fp64", "--step", "3", "--temporal", "force", "--prefetch", "--bx", "34", "--by", "8", "--block-merge-y", "2", "--sn", "16"]
ROWS = ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "16", "--prefetch", "--order", "rows"]
TILE = ["--dtype", "fp32"]
STREAM = ["--dtype", "fp64", "--streaming", "--prefetch"]
BASES = {"d3": (D3, "smoke3"), "d3f64": (D3F64, "t3_star"), "pipe": (PIPE, "t3_star"), "rows": (ROWS, "smoke3"), "tile": (TILE, "t2_box9"),
         "stream": (STREAM, "t2_star"), "cross": (["--3d", "--dtype", "fp32", "--dist", "2"], "t3_cross"),
         "odd": (["--3d", "--dtype", "fp32", "--step", "2"], "t3_star_odd")}     # N = 263: element-wide accesses
ALL = tuple(BASES)
KNOBS = [(["--xcd-remap", str(n)], ALL) for n in range(6)] + [
    (["--xcd-remap", "3", "--zgroup", "2"], ("d3",)), (["--xcd-remap", "5", "--xcd-chunk", "3"], ("d3", "tile")),
] + [(["--schedule", s, "--lazy-rims", lz], ("d3", "d3f64", "stream", "cross")) for s in ("window", "reuse") for lz in ("0", "1")] + [
    (["--schedule", "reuse", "--dist", "1", "--merge-forward", mf], ("d3", "cross")) for mf in ("0", "100")] + [
    (["--stage", "dma"], ("d3", "d3f64", "stream", "cross", "rows")), (["--stage", "dma", "--loader-waves", "2"], ("d3", "d3f64", "stream")),
    (["--stage", "dma", "--loader-waves", "1", "--prefetch-depth", "1"], ("d3",)), (["--stage", "dma", "--schedule", "window"], ("d3", "cross")),
    (["--stage", "dma", "--xrim", "lds"], ("d3",)), (["--stage", "dma", "--store-mask", "buffer", "--defer-stores", "1"], ("d3",)),
    (["--skew", "1"], ("pipe", "d3")), (["--skew", "2"], ("pipe",)), (["--skew", "0"], ("pipe",)),
    (["--skew", "2", "--order", "rows"], ("pipe",)), (["--skew", "1", "--order", "rows", "--pack", "1", "--dtype", "fp32"], ("pipe",)),
    (["--temporal", "1"], ("d3", "stream")), (["--temporal", "force", "--exact-y", "1"], ("d3",)),
    (["--defer-stores", "1"], ("d3", "d3f64", "stream", "cross")), (["--drain", "1"], ("d3", "pipe")), (["--drain", "2"], ("d3", "pipe")),
    (["--uniform-loads", "1"], ("d3", "stream", "pipe")), (["--uniform-loads", "2"], ("d3", "stream", "pipe")),
    (["--uniform-loads", "2", "--store-mask", "buffer"], ("d3", "d3f64", "rows")), (["--store-mask", "buffer"], ALL),
    (["--store-mask", "buffer", "--clamp-loads", "0"], ("d3", "tile")), (["--coef", "sgpr"], ("d3", "rows", "tile", "d3f64")),
    (["--coef", "vgpr"], ("d3",)), (["--cyclic-merge-x", "4"], ("d3", "tile", "stream", "cross")), (["--cyclic-merge-x", "4", "--xrim", "lds"], ("d3",)),
    (["--cyclic-merge-y", "2"], ("d3", "tile", "rows")), (["--zigzag", "1"], ("d3", "stream", "tile")),
    (["--xedge-select", "1"], ("d3", "tile", "cross")), (["--halo-spread", "1"], ("d3", "tile", "d3f64")), (["--xrim", "lds"], ALL),
] + [(["--nt-load", n], ("d3", "tile")) for n in "123"] + [(["--nt-store", n], ("d3", "tile")) for n in ("0", "1", "16")] + [
    (["--nt-store", "16", "--store-mask", "buffer", "--nt-load", "1"], ("d3",)), (["--waves-per-eu", "2"], ("d3", "tile")),
    (["--rot-mod", "8"], ("d3", "rows")), (["--rot-mod", "6"], ("rows",)), (["--stream-unroll", "8"], ("d3", "rows")),
    (["--order", "rows", "--pack", "1", "--block-merge-x", "2"], ("d3", "tile")), (["--order", "rows", "--pack", "1", "--block-merge-x", "4"], ("d3", "tile")),
    (["--order", "rows", "--pack", "0"], ("d3", "tile", "stream", "d3f64")), (["--pack", "1", "--xrim", "lds"], ("rows",)),
    (["--row-fence", "-1"], ("rows",)), (["--row-fence", "7"], ("rows",)), (["--pin", "1"], ("d3", "pipe")), (["--pin", "0"], ("rows", "pipe")),
] + [(["--debug-skip", str(b)], ("d3", "tile", "rows")) for b in (1, 2, 4, 8, 15)] + [
    (["--debug-drop-barrier", "1"], ("pipe",)), (["--debug-drop-barrier", "2"], ("d3", "cross")),
    (["--clamp-loads", "0"], ("d3", "tile", "stream", "pipe")), (["--exact-x", "0"], ("d3", "tile")), (["--exact-y", "0"], ("d3", "tile")),
    (["--exact-y", "1"], ("pipe",)), (["--prefetch-depth", "2"], ("d3", "pipe", "rows")), (["--prefetch-depth", "4"], ("d3",)),
    (["--prefetch-auto", "0"], (["--3d", "--dtype", "fp32", "--step", "2"],)), (["--lds-pad", "3"], ("d3", "tile")), (["--out-skew", "8"], ("d3",)),
    (["--cc-opt", "-fno-slp-vectorize"], ("d3",)), (["--ref-defaults"], ("d3", "tile", "cross")), (["--pair-launch", "1"], ("d3", "stream")),
    (["--time-order", "2"], ("d3f64", "tile", "cross")), (["--boundary", "periodic"], ("d3f64", "tile", "stream")),
    (["--step", "3"], ("d3f64", "tile")), (["--tuned-defaults", "0"], ("d3f64",)),
]


def knob_lists():
    out = []
    for words, bases in KNOBS:
        for b in bases:
            opts, name = BASES[b] if isinstance(b, str) else (b, "t3_star")
            out.append((None, list(opts) + list(words) + [stc(name)]))
    return out


def host_lists():
    """The emitted main(): N-GPU hosts, the pair launch, --check with periodic boundaries and second-order time stepping."""
    wave3 = ["--3d", "--dtype", "fp32", "--time-order", "2", "--check"]
    return [(None, l) for l in [
        ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "16", "--gpus", "2", "--check", stc("t3_star")],
        ["--3d", "--dtype", "fp64", "--gpus", "8", stc("t3_star")],
        ["--dtype", "fp32", "--streaming", "--step", "2", "--sn", "16", "--gpus", "2", "--check", stc("t2_star")],
        ["--3d", "--dtype", "fp32", "--sn", "8", "--pair-launch", "1", stc("t3_star")],
        # periodic: rows of a multiple of 16 bytes (the wrap kernel copies vectors) and not
        ["--3d", "--dtype", "fp32", "--boundary", "periodic", "--check", stc("smoke3")],
        ["--3d", "--dtype", "fp32", "--boundary", "periodic", "--check", stc("t3_star")],
        ["--3d", "--dtype", "fp64", "--boundary", "periodic", "--check", stc("t3_star_odd")],
        ["--dtype", "fp32", "--boundary", "periodic", "--check", stc("t2_box9")],
        ["--dtype", "fp32", "--boundary", "periodic", "--check", stc("t2_star")],
        ["--dtype", "fp64", "--boundary", "periodic", "--check", stc("t2_odd")],
        wave3 + [stc("t3_wave")], wave3 + ["--store-mask", "buffer", stc("t3_wave")],
        wave3 + ["--prefetch", "--prefetch-depth", "1", stc("t3_wave")], wave3 + ["--prefetch", "--prefetch-depth", "2", stc("t3_wave")],
        wave3 + ["--prefetch", "--prefetch-depth", "2", "--store-mask", "buffer", stc("t3_wave")],
        ["--dtype", "fp64", "--time-order", "2", "--check", stc("t2_wave")],
        # rejected before the emitter is asked
        ["--3d", "--boundary", "periodic", "--gpus", "2", stc("t3_star")], ["--3d", "--time-order", "2", "--pair-launch", "1", stc("t3_wave")],
        ["--3d", "--gpus", "65", stc("t3_star")], ["--3d", "--bogus", stc("t3_star")], ["--3d", "--step", stc("t3_star")],
        ["--3d", stc("no_such_spec")], ["--help"],
    ]]


def boundary_lists():
    """--boundary reflect and --boundary-x / -y / -z.  Last in the corpus, so that the lists in front keep their numbers: against a build
    without these options `diff -r` shows these files and nothing else."""
    return [(None, l) for l in [
        # reflecting and per-axis boundaries: vector and element rows, 2D, a fixed x, the canonical spelling, order 2 in a rigid box
        ["--3d", "--dtype", "fp32", "--boundary", "reflect", "--check", stc("smoke3")],
        ["--3d", "--dtype", "fp64", "--step", "2", "--boundary", "reflect", stc("t3_star_odd")],
        ["--3d", "--dtype", "fp32", "--boundary-z", "fixed", "--boundary-y", "periodic", "--boundary-x", "reflect", stc("t3_star")],
        ["--3d", "--dtype", "fp64", "--boundary", "reflect", "--boundary-x", "fixed", stc("t3_star")],
        ["--3d", "--dtype", "fp32", "--boundary-x", "periodic", "--boundary-y", "periodic", "--boundary-z", "periodic", stc("t3_star")],
        ["--dtype", "fp32", "--boundary-y", "periodic", "--boundary-x", "reflect", "--check", stc("t2_star")],
        ["--dtype", "fp64", "--boundary", "reflect", stc("t2_odd")],
        ["--3d", "--dtype", "fp32", "--time-order", "2", "--boundary", "reflect", stc("t3_wave")],
        # rejected before the emitter is asked
        ["--3d", "--boundary", "reflect", "--gpus", "2", stc("t3_star")], ["--3d", "--boundary-y", "periodic", "--pair-launch", "1", stc("t3_star")],
        ["--boundary-z", "reflect", stc("t2_star")], ["--3d", "--boundary-x", "torus", stc("t3_star")],
    ]] + [(None, j) for j in __import__("boundary_cases").all_build_args()]       # what build() emits for the boundary tests


def source_lists():
    """--source.  Behind everything else, so that the lists in front keep their numbers: against a build without the option `diff -r`
    shows these files (and --help) and nothing else."""
    import source_cases
    src3 = ["--3d", "--dtype", "fp32", "--source", "--check"]
    lists = [
        # the emitted main() with a third array, every issue point of the stream, both extra streams at once, the knob bases
        src3 + [stc("t3_wave")], src3 + ["--store-mask", "buffer", stc("t3_wave")],
        src3 + ["--prefetch", "--prefetch-depth", "2", stc("t3_wave")], src3 + ["--prefetch", "--prefetch-depth", "2", "--store-mask", "buffer", stc("t3_wave")],
        src3 + ["--time-order", "2", "--prefetch", "--prefetch-depth", "2", stc("t3_wave")], src3 + ["--stage", "dma", stc("t3_wave")],
        src3 + ["--order", "rows", "--pack", "1", "--block-merge-x", "4", "--defer-stores", "1", "--prefetch", stc("t3_wave")],
        ["--dtype", "fp64", "--source", "--time-order", "2", "--check", stc("t2_wave")], ["--dtype", "fp32", "--source", "--boundary", "reflect", stc("t2_star")],
        ["--dtype", "fp64", "--source", "--streaming", "--stage", "dma", stc("t2_star")],
        # rejected before the emitter is asked
        ["--3d", "--source", "--step", "2", stc("t3_star")], ["--3d", "--source", "--step", "2", "--temporal", "1", stc("t3_star")],
        ["--3d", "--source", "--temporal", "force", stc("t3_star")], ["--3d", "--source", "--gpus", "2", stc("t3_star")],
        ["--3d", "--source", "--pair-launch", "1", stc("t3_star")],
    ]
    for b in ("d3f64", "tile", "cross", "stream"):
        opts, name = BASES[b]
        lists.append(list(opts) + ["--source", stc(name)])
    return [(None, l) for l in lists] + [(None, j) for j in source_cases.all_build_args()]       # what build() emits for the source tests


def residual_lists():
    """--residual max.  Behind everything else, so that the lists in front keep their numbers: against a build without the option `diff -r`
    shows these files (and --help) and nothing else."""
    import residual_cases
    res3 = ["--3d", "--dtype", "fp32", "--residual", "max", "--check"]
    lists = [
        # the emitted main() with the residual array, every issue point of the centre stream, all three streams at once, the knob bases
        res3 + [stc("t3_wave")], res3 + ["--store-mask", "buffer", stc("t3_wave")],
        res3 + ["--prefetch", "--prefetch-depth", "2", stc("t3_wave")], res3 + ["--source", "--time-order", "2", "--prefetch", "--prefetch-depth", "2", stc("t3_wave")],
        ["--3d", "--dtype", "fp64", "--residual", "max", "--check", "--stage", "dma", "--loader-waves", "1", stc("t3_star")], res3 + ["--step", "2", stc("t3_star")],
        ["--dtype", "fp64", "--residual", "max", "--check", stc("t2_wave")], ["--dtype", "fp64", "--residual", "max", "--streaming", "--stage", "dma", stc("t2_star")],
        # rejected before the emitter is asked
        ["--3d", "--residual", "l2", stc("t3_star")], ["--3d", "--residual", "max", "--step", "2", "--temporal", "1", stc("t3_star")],
        ["--3d", "--residual", "max", "--gpus", "2", stc("t3_star")], ["--3d", "--residual", "max", "--pair-launch", "1", stc("t3_star")],
    ]
    for b in ("d3", "d3f64", "rows", "tile", "cross", "stream", "odd"):
        opts, name = BASES[b]
        lists.append(list(opts) + ["--residual", "max", stc(name)])
    return [(None, l) for l in lists] + [(None, j) for j in residual_cases.all_build_args()]       # what build() emits for the residual tests


def dirichlet_lists():
    """--dirichlet.  Behind everything else, so that the lists in front keep their numbers: against a build without the option `diff -r`
    shows these files (and --help) and nothing else."""
    import dirichlet_cases
    fix3 = ["--3d", "--dtype", "fp32", "--dirichlet", "--check"]
    lists = [
        # the emitted main() with the array of held cells, every issue point of the fix stream, all four streams at once, the knob bases
        fix3 + [stc("t3_wave")], fix3 + ["--store-mask", "buffer", stc("t3_wave")],
        fix3 + ["--prefetch", "--prefetch-depth", "2", stc("t3_wave")], fix3 + ["--prefetch", "--prefetch-depth", "2", "--store-mask", "buffer", stc("t3_wave")],
        fix3 + ["--source", "--time-order", "2", "--residual", "max", "--prefetch", "--prefetch-depth", "2", stc("t3_wave")], fix3 + ["--stage", "dma", stc("t3_wave")],
        fix3 + ["--order", "rows", "--pack", "1", "--block-merge-x", "4", "--defer-stores", "1", "--prefetch", stc("t3_wave")],
        ["--dtype", "fp64", "--dirichlet", "--time-order", "2", "--check", stc("t2_wave")], ["--dtype", "fp32", "--dirichlet", "--boundary", "reflect", stc("t2_star")],
        ["--dtype", "fp64", "--dirichlet", "--streaming", "--stage", "dma", stc("t2_star")],
        # the option has one place in the banner
        ["--dirichlet", "--3d", "--dirichlet", "--dtype", "fp32", stc("t3_wave")],
        # rejected before the emitter is asked
        ["--3d", "--dirichlet", "--step", "2", stc("t3_star")], ["--3d", "--dirichlet", "--step", "2", "--temporal", "1", stc("t3_star")],
        ["--3d", "--dirichlet", "--temporal", "force", stc("t3_star")], ["--3d", "--dirichlet", "--gpus", "2", stc("t3_star")],
        ["--3d", "--dirichlet", "--pair-launch", "1", stc("t3_star")],
    ]
    for b in ("d3", "d3f64", "rows", "tile", "cross", "stream", "odd"):
        opts, name = BASES[b]
        lists.append(list(opts) + ["--dirichlet", stc(name)])
    return [(None, l) for l in lists] + [(None, j) for j in dirichlet_cases.all_build_args()]       # what build() emits for the dirichlet tests


def scale_lists():
    """--scale and --scale-centre.  Behind everything else, so that the lists in front keep their numbers: against a build without the
    options `diff -r` shows these files (and --help) and nothing else."""
    import scale_cases
    scl3 = ["--3d", "--dtype", "fp32", "--scale", "--check"]
    cen = ["--scale-centre", "0.3"]
    lists = [
        # the emitted main() with the array of factors, every issue point of the scale stream, with and without a centre term, all six
        # streams at once, the centre stream shared with the residual, the knob bases
        scl3 + [stc("t3_wave")], scl3 + cen + [stc("t3_wave")], scl3 + ["--store-mask", "buffer", stc("t3_wave")], scl3 + cen + ["--store-mask", "buffer", stc("t3_wave")],
        scl3 + ["--prefetch", "--prefetch-depth", "2", stc("t3_wave")], scl3 + cen + ["--prefetch", "--prefetch-depth", "2", "--store-mask", "buffer", stc("t3_wave")],
        scl3 + cen + ["--source", "--time-order", "2", "--residual", "max", "--dirichlet", "--prefetch", "--prefetch-depth", "2", stc("t3_wave")],
        scl3 + cen + ["--residual", "max", stc("t3_wave")], scl3 + ["--residual", "max", stc("t3_wave")], scl3 + cen + ["--stage", "dma", stc("t3_wave")],
        scl3 + cen + ["--order", "rows", "--pack", "1", "--block-merge-x", "4", "--defer-stores", "1", "--prefetch", stc("t3_wave")],
        ["--dtype", "fp64", "--scale", "--scale-centre", "2", "--time-order", "2", "--check", stc("lap2")], ["--dtype", "fp32", "--scale", "--scale-centre", "1", "--boundary", "reflect", stc("lap2")],
        ["--dtype", "fp64", "--scale", "--scale-centre", "-1.5", "--streaming", "--stage", "dma", stc("t2_star")],
        # the options have one place in the banner; the centre as a coefficient is written; 0 leaves no trace
        ["--scale", "--3d", "--scale-centre", "0.30000001", "--scale", "--dtype", "fp32", stc("t3_wave")], ["--scale-centre", "0", "--3d", "--scale", "--dtype", "fp32", stc("t3_wave")],
        # rejected before the emitter is asked
        ["--3d", "--scale", "--step", "2", stc("t3_star")], ["--3d", "--scale", "--step", "2", "--temporal", "1", stc("t3_star")],
        ["--3d", "--scale", "--temporal", "force", stc("t3_star")], ["--3d", "--scale", "--gpus", "2", stc("t3_star")],
        ["--3d", "--scale", "--pair-launch", "1", stc("t3_star")], ["--3d", "--scale-centre", "1", stc("t3_star")], ["--3d", "--scale", "--scale-centre", "nan", stc("t3_star")],
    ]
    for b in ("d3", "d3f64", "rows", "tile", "cross", "stream", "odd"):
        opts, name = BASES[b]
        lists.append(list(opts) + ["--scale", "--scale-centre", "1", stc(name)])
    return [(None, l) for l in lists] + [(None, j) for j in scale_cases.all_build_args()]       # what build() emits for the scale tests


def varcoef_lists():
    """--varcoef.  Behind everything else, so that the lists in front keep their numbers: against a build without the option `diff -r`
    shows these files (and --help) and nothing else."""
    import varcoef_cases
    vc3 = ["--3d", "--dtype", "fp32", "--varcoef", "--check"]
    cfg = os.path.join(ROOT, "benchmarks", "configs")
    lists = [
        # the emitted main() with the coefficient grids, every issue point of the coefficient loads, a sum that starts late, five leads,
        # the reuse and window schedules, all streams at once
        vc3 + [stc("t3_wave")], vc3 + ["--store-mask", "buffer", stc("t3_wave")], vc3 + ["--prefetch", "--prefetch-depth", "2", stc("t3_wave")],
        vc3 + ["--stage", "dma", stc("t3_wave")], vc3 + ["--order", "rows", "--defer-stores", "1", "--prefetch", stc("t3_wave")],
        vc3 + ["--by", "4", "--block-merge-y", "2", stc("t3_ahead")], vc3 + ["--by", "8", "--block-merge-y", "1", stc("shape_11_3d_o2")],
        vc3 + ["--dist", "1", stc("t3_wave")], vc3 + ["--schedule", "window", stc("t3_wave")],
        vc3 + ["--source", "--time-order", "2", "--residual", "max", "--dirichlet", "--scale", "--scale-centre", "0.3", "--prefetch", stc("t3_wave")],
        ["--dtype", "fp64", "--varcoef", "--check", stc("lap2")], ["--dtype", "fp32", "--varcoef", "--streaming", "--boundary", "reflect", stc("t2_ahead")],
        ["--dtype", "fp64", "--varcoef", "--streaming", "--stage", "dma", stc("t2_box25")],
        # the option has one place in the banner; the bare benchmark commands (the fit rule)
        ["--varcoef", "--3d", "--varcoef", "--dtype", "fp32", stc("t3_wave")],
        ["--dtype", "fp32", "--varcoef", os.path.join(cfg, "c1_2d5pt_star_4096.stc")], ["--dtype", "fp32", "--varcoef", os.path.join(cfg, "c2_2d5pt_star_8192.stc")],
        ["--3d", "--dtype", "fp32", "--varcoef", os.path.join(cfg, "c3_3d7pt_star_512.stc")], ["--3d", "--dtype", "fp32", "--varcoef", os.path.join(cfg, "c4_3d7pt_star_1024.stc")],
        ["--dtype", "fp64", "--varcoef", os.path.join(cfg, "c5_2d25pt_box_16384.stc")],
        # rejected before the emitter is asked
        ["--3d", "--varcoef", "--step", "2", stc("t3_star")], ["--3d", "--varcoef", "--temporal", "force", stc("t3_star")], ["--3d", "--varcoef", "--gpus", "2", stc("t3_star")],
        ["--3d", "--varcoef", "--pair-launch", "1", stc("t3_star")], ["--3d", "--dtype", "fp32", "--varcoef", "--coef", "sgpr", stc("t3_star")],
        ["--3d", "--dtype", "fp32", "--varcoef", "--order", "rows", "--pack", "1", stc("t3_star")],
    ]
    for b in ("d3", "d3f64", "rows", "tile", "cross", "stream", "odd"):
        opts, name = BASES[b]
        if "--pack" not in opts:
            lists.append(list(opts) + ["--varcoef", stc(name)])
    return [(None, l) for l in lists] + [(None, j) for j in varcoef_cases.all_build_args()]       # what build() emits for the varcoef tests


def interface_lists():
    """The launch interfaces (csrc/plan.hpp: LaunchAbi).  What the lists in front leave open of: every one of the nine interfaces with and
    without --check, in 2D and in 3D; a ring fill in front of the widest signature; every row of the generator's refusal table with
    --gpus 2 and with --pair-launch 1.  --coverage counts them.  Behind everything else, so that the lists in front keep their numbers."""
    every = ["--scale", "--varcoef", "--source", "--residual", "max", "--dirichlet"]
    fsr = ["--dirichlet", "--source", "--residual", "max"]
    d2, d3 = ["--dtype", "fp64"], ["--3d", "--dtype", "fp32"]
    return [(None, l) for l in [
        d2 + ["--residual", "max", "--source", "--check", stc("poisson2")],
        d2 + fsr + ["--check", stc("t2_wave")], d2 + fsr + [stc("t2_star")], d2 + fsr + ["--streaming", stc("t2_star")],
        d2 + every + ["--check", stc("lap2")], d2 + every + [stc("lap2")], d3 + every + [stc("t3_wave")],
        d3 + every + ["--boundary", "periodic", "--check", stc("t3_wave")], d2 + every + ["--boundary-x", "reflect", stc("lap2")],
        # rejected before the emitter is asked: the rows of the refusal table the lists in front do not reach, and both options at once
        ["--3d", "--time-order", "2", "--gpus", "2", stc("t3_wave")], ["--3d", "--boundary", "periodic", "--pair-launch", "1", stc("t3_star")],
        ["--3d", "--source", "--gpus", "2", "--pair-launch", "1", stc("t3_star")], ["--3d", "--dirichlet", "--scale", "--varcoef", "--pair-launch", "1", stc("t3_star")],
    ]]


def corpus():
    return build_lists() + space_sample() + host_lists() + knob_lists() + boundary_lists() + source_lists() + residual_lists() + dirichlet_lists() + scale_lists() + varcoef_lists() + interface_lists()


def coverage(lists):
    """Lists of the corpus per option value named in KNOBS (first word pair of each entry)."""
    seen = {}
    for words, _ in KNOBS:
        for i in range(0, len(words) - 1, 2):
            seen.setdefault((words[i], words[i + 1]), 0)
    for _, l in lists:
        for i in range(len(l) - 1):
            if (l[i], l[i + 1]) in seen:
                seen[(l[i], l[i + 1])] += 1
    return seen


INTERFACES = {"plain": (), "source": ("--source",), "residual": ("--residual",), "residual+source": ("--residual", "--source"), "dirichlet": ("--dirichlet",),
              "dirichlet+source+residual": ("--dirichlet", "--source", "--residual"), "scale": ("--scale",), "varcoef": ("--varcoef",),
              "scale+varcoef+source+residual+dirichlet": ("--scale", "--varcoef", "--source", "--residual", "--dirichlet")}
ARRAY_OPTIONS = ("--source", "--residual", "--dirichlet", "--scale", "--varcoef")
REFUSAL_ROWS = {"ring fill, periodic": lambda l: "--boundary periodic" in " ".join(l), "ring fill, other": lambda l: "--boundary" in " ".join(l) and "--boundary periodic" not in " ".join(l),
                "time order": lambda l: "--time-order 2" in " ".join(l), "source": lambda l: "--source" in l, "residual": lambda l: "--residual" in l,
                "dirichlet": lambda l: "--dirichlet" in l, "varcoef": lambda l: "--varcoef" in l, "scale": lambda l: "--scale" in l}


def interface_coverage(lists):
    """Per launch interface: lists with / without --check in 2D / 3D; per row of the refusal table: lists with --gpus N and with --pair-launch 1;
    lists with --pair-launch 1; lists with a ring fill in front of each family's entry points."""
    out = []
    for name, words in INTERFACES.items():
        mine = [l for _, l in lists if {w for w in l if w in ARRAY_OPTIONS} == set(words) and "--gpus" not in l and "--pair-launch" not in l and "--temporal" not in l]
        n = {(c, d): sum(1 for l in mine if ("--check" in l) == c and ("--3d" in l) == d) for c in (True, False) for d in (True, False)}
        out.append("%-42s --check 2D %3d  3D %3d   plain 2D %3d  3D %3d   ring fill %3d" % (name, n[True, False], n[True, True], n[False, False], n[False, True],
                                                                                             sum(1 for l in mine if any(w.startswith("--boundary") for w in l))))
    for name, has in REFUSAL_ROWS.items():
        out.append("refused: %-22s --gpus N %3d   --pair-launch 1 %3d" % (name, sum(1 for _, l in lists if has(l) and "--gpus" in l), sum(1 for _, l in lists if has(l) and "--pair-launch" in l)))
    out.append("--pair-launch 1 emitted lists: %d" % sum(1 for _, l in lists if "--pair-launch" in l and not any(w in l for w in ARRAY_OPTIONS + ("--boundary", "--time-order"))))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("outdir")
    ap.add_argument("--lib", default=os.path.join(ROOT, "drstencil_amd", "libdrstencil_amd.so"))
    ap.add_argument("--cli", default=None, help="drstencil binary of the same build (default: bin/drstencil two levels above --lib)")
    ap.add_argument("--coverage", action="store_true")
    a = ap.parse_args()
    cli = a.cli or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(a.lib))), "bin", "drstencil")
    L = ctypes.CDLL(os.path.abspath(a.lib))
    L.drs_generate.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]
    L.drs_free.argtypes = [ctypes.c_void_p]

    def take(p):
        s = ctypes.string_at(p.value) if p.value else None
        if p.value:
            L.drs_free(p.value)
        return s

    lists = corpus()
    os.makedirs(a.outdir, exist_ok=True)
    home = os.getcwd()
    emitted = rejected = 0
    with open(os.path.join(a.outdir, "MANIFEST"), "w") as man:
        for n, (cwd, args) in enumerate(lists):
            os.chdir(cwd or home)
            arr = (ctypes.c_char_p * len(args))(*[os.fsencode(x) for x in args])
            src, msg = ctypes.c_void_p(), ctypes.c_void_p()
            rc = L.drs_generate(len(args), arr, ctypes.byref(src), ctypes.byref(msg))
            source, messages = take(src), take(msg) or b""
            text = b"args: " + " ".join(args).encode() + b"\nexit code: %d\nmessages:\n" % rc + messages
            if source is None:
                # why: the command's stderr (nothing is written: a rejected list emits no file)
                r = subprocess.run([cli] + args, capture_output=True, cwd=cwd or home)
                text += b"stderr (exit code %d):\n" % r.returncode + r.stderr
                rejected += 1
            else:
                text += b"source:\n" + source
                emitted += 1
            os.chdir(home)
            with open(os.path.join(a.outdir, "%04d.txt" % n), "wb") as f:
                f.write(text)
            man.write("%s  %04d  %s\n" % (hashlib.sha256(text).hexdigest(), n, " ".join(args)))
    digest = hashlib.sha256(open(os.path.join(a.outdir, "MANIFEST"), "rb").read()).hexdigest()
    print("%d configurations: %d emitted, %d rejected; MANIFEST sha256 %s" % (len(lists), emitted, rejected, digest))
    if a.coverage:
        for (k, v), c in sorted(coverage(lists).items()):
            print("%4d  %s %s" % (c, k, v))
        print("\n".join(interface_coverage(lists)))


if __name__ == "__main__":
    main()
