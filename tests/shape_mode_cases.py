"""Random stencil shapes in every problem mode (tests/test_shape_modes_cpu.py, tests/test_shape_modes_gpu.py): a seeded sample of 12
point sets from fuzz_shapes.random_shape -- sparse to dense, one-sided along the streamed dimension (four of the 12), without a centre (six),
mixed-sign coefficients (five; none of the 12 drew a duplicate offset); 2D and 3D, orders 1 and 2 -- committed as tests/stc/shape_*.stc (draw_shapes wrote them; the files are the
sample, so the cases and the kernel cache keys do not depend on how the shapes were drawn), and for every shape one random
configuration of the tuner's space per mode:
    fixed, periodic, reflect, mixed (a seeded per-axis triple, boundary_cases.mode_triple): steps 1 to 3, on-chip stages allowed
    order2, source, order2_source, order2_source_mixed (--time-order 2 --source with a per-axis triple): step 1, no on-chip stages
The hand-drawn stars, boxes and crosses of every other mode test have their taps on both sides of the output plane; the old-value and
source streams are issued a prefetch distance ahead of the iteration that completes an output plane, and which iteration that is
depends on the shape's extent along the streamed dimension.

The committed grids are fuzz_shapes' small ones: several stream blocks under most configurations, a partial x-edge tile, row lengths
that are multiples of 16 bytes in some shapes and not in others, every axis at least 3 Halo of the deepest step drawn.  The emulated
suite runs the same shapes on tiny ragged grids (the ranges of test_emulated_kernels._random_shape_jobs).

Every GPU kernel is prebuilt by __graft_entry__.build().  Refusals are decided when build() compiles (the runtime refuses kernels that
spill, the generator rejects a --dist the shape has no data to reuse at, an LDS demand beyond the limit or LDS-DMA staging on rows that
are no multiple of the 16-byte vector), so they are known before any GPU run.  Cross-compiling for gfx950, build() printed:
    shape fuzz fixed: 10 kernels built, 2 refused
    shape fuzz periodic: 10 kernels built, 2 refused
    shape fuzz reflect: 11 kernels built, 1 refused
    shape fuzz mixed: 11 kernels built, 1 refused
    shape fuzz order2: 9 kernels built, 3 refused
    shape fuzz source: 10 kernels built, 2 refused
    shape fuzz order2_source: 10 kernels built, 2 refused
    shape fuzz order2_source_mixed: 11 kernels built, 1 refused
(6 for a --dist without data to reuse, 6 for register spills, 2 for an LDS demand beyond 160 KiB).  The emulated suite asserts that the
generator rejects at most a quarter of each mode's 12 on its tiny grids, the GPU suite at least MIN_CHECKED of each mode's 12 checked.
"""
import glob
import os
import random

from shape_knobs import config_options, legal_dists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STC = os.path.join(ROOT, "tests", "stc")

MODES = ("fixed", "periodic", "reflect", "mixed", "order2", "source", "order2_source", "order2_source_mixed")
STEP1 = ("order2", "source", "order2_source", "order2_source_mixed")
MODE_OPTS = {"fixed": [], "periodic": ["--boundary", "periodic"], "reflect": ["--boundary", "reflect"], "mixed": [],
             "order2": ["--time-order", "2"], "source": ["--source"], "order2_source": ["--time-order", "2", "--source"],
             "order2_source_mixed": ["--time-order", "2", "--source"]}
TRIPLE = ("mixed", "order2_source_mixed")       # a per-axis boundary triple is appended
SHAPE_SEED = 7
N_SHAPES = 12
MIN_CHECKED = 9                                 # three quarters of a mode's sample
# The seed of the configurations: the first for which __graft_entry__.build() -- the generator and the compiler, no GPU and no result
# of a kernel involved -- builds at least MIN_CHECKED kernels of every mode; "mixed" got 7 of 12 with it and takes the next seed that
# gives it more than 9.
CONFIG_SEED = 2
MODE_SEED = {"mixed": 4}
MAX_TAPS = 64                                   # fused point count above which a step above 1 is not drawn: beyond it most kernels of these dense
                                                # shapes spill (the runtime refuses them) and take minutes to compile; fuzz_shapes.py goes to 420


def shape_files():
    return sorted(glob.glob(os.path.join(STC, "shape_*.stc")))


def shape_points(path, ndim):
    """[(offsets..., coefficient)] as the file lists them (duplicates kept), and whether the coefficients have both signs."""
    pts, seen = [], False
    for ln in open(path).read().splitlines():
        if ln.strip() == "stencil":
            seen = True
        elif seen and ln.split():
            f = ln.split()
            pts.append(tuple(int(x) for x in f[:ndim]) + (float(f[ndim]),))
    return pts, any(p[-1] < 0 for p in pts) and any(p[-1] > 0 for p in pts)


def shapes():
    """[(name, ndim, order, path)] of the committed sample, from the file names (shape_<nn>_<ndim>d_o<order>.stc)."""
    out = []
    for p in shape_files():
        name = os.path.basename(p)[:-4]
        _, _, nd, o = name.split("_")
        out.append((name, int(nd[0]), int(o[1:]), p))
    return out


def traits(pts, ndim):
    """(one-sided along the streamed dimension, without a centre) of a point set."""
    return all(p[0] >= 0 for p in pts) or all(p[0] <= 0 for p in pts), not any(all(x == 0 for x in p[:ndim]) for p in pts)


def draw_shapes(out_dir=STC, seed=SHAPE_SEED):
    """Write the sample (run once, by hand: python tests/shape_mode_cases.py): N_SHAPES shapes from fuzz_shapes.random_shape, 2D and
    3D alternating, order 2 for every third, on fuzz_shapes' small grids; drawn again until the sample holds at least two shapes that
    are one-sided along the streamed dimension and two without a centre, between 3 and 9 row lengths that are multiples of 4 elements,
    and no shape without two points behind one another along the streamed dimension (every --dist of such a shape is refused)."""
    import fuzz_shapes as fs
    from helpers import write_stc
    rnd = random.Random(seed)
    while True:
        drawn = []
        for s in range(N_SHAPES):
            ndim = 3 if s % 2 else 2
            h = 2 if s % 3 == 2 else 1
            pts, _ = fs.random_shape(rnd, ndim, h)
            dims = (rnd.randint(18 + 2 * h, 40), rnd.randint(30, 70), rnd.randint(130, 300)) if ndim == 3 else (1, rnd.randint(90, 260), rnd.randint(200, 600))
            drawn.append((s, ndim, h, pts, dims, rnd.randint(2, 6)))
        tr = [traits(d[3], d[1]) for d in drawn]
        vec = [d[4][2] % 4 == 0 for d in drawn]
        reuse = all(legal_dists(d[3], 1) for d in drawn)      # else every --dist is refused: "No data to reuse"
        if reuse and sum(a for a, _ in tr) >= 2 and sum(b for _, b in tr) >= 2 and 3 <= sum(vec) <= N_SHAPES - 3:
            break
    for s, ndim, h, pts, dims, iters in drawn:
        write_stc(os.path.join(out_dir, "shape_%02d_%dd_o%d.stc" % (s, ndim, h)), ndim, dims, iters, pts)
    return drawn


def emulated_dims(name, ndim, h):
    """The tiny ragged grid of a shape in the emulated suite (seeded by the shape's name; test_emulated_kernels._random_shape_jobs'
    ranges)."""
    rnd = random.Random("shape-modes/dims/" + name)
    return (rnd.randint(6 + 4 * h, 14), rnd.randint(9 + 4 * h, 24), rnd.randint(40, 150)) if ndim == 3 else (1, rnd.randint(20, 50), rnd.randint(40, 280))


def sample_jobs(mode, emulated=False):
    """One job per committed shape in `mode`: (id, ndim, stc, dims, dtype, options without the .stc, step).  dims: the grid the job
    runs on -- the file's own (GPU) or emulated_dims (the caller writes the shape's points on it).  The configuration is the first of
    a seeded draw from the tuner's space, with fuzz_shapes' random knobs, that the tuner's spill model lets through (GPU; as
    fuzz_shapes.make_jobs does) or that fits the emulator (workgroups of at most 256 lanes), LDS-DMA staging left to the grids
    whose rows are multiples of 16 bytes; the steps drawn are those whose fused
    point count stays below MAX_TAPS and whose Halo fits three times into every axis, so that every mode's grid allows its job."""
    import oracle
    from boundary_cases import mode_triple
    from drstencil_amd.tuner import tuning as t
    assert mode in MODES, mode
    jobs = []
    for n, (name, ndim, h, path) in enumerate(shapes()):
        pts, mixed = shape_points(path, ndim)
        dims = emulated_dims(name, ndim, h) if emulated else oracle.Spec(path, ndim, 1).dims
        shape = dims[3 - ndim:]
        dtype = ("fp32", "fp64")[(n + MODES.index(mode)) % 2]
        distinct = len(set(p[:-1] for p in pts))
        steps = tuple(st for st in ((1,) if mode in STEP1 else (1, 2) if emulated else (1, 2, 3))
                      if (st == 1 or min((2 * h * st + 1) ** ndim, distinct ** st) <= MAX_TAPS) and min(shape) >= 3 * h * st)
        rnd = random.Random("shape-modes/%s/%s/%d%s" % (name, mode, MODE_SEED.get(mode, CONFIG_SEED), "/emulated" if emulated else ""))
        t.order, t.ndim, t.elem_bytes = h, ndim, 4 if dtype == "fp32" else 8
        space = t.enumerate_space(steps)
        if emulated:
            space = [v for v in space if v[2][0] * v[2][1] <= 256 and v[2][0] <= 68 and v[3] <= 16]
        dists, job = {}, None
        for v in rnd.sample(space, min(len(space), 32)):
            cl = config_options(rnd, v, ndim, h, pts, mixed, dists)
            if cl is None:
                continue
            if "--stage" in cl and (shape[-1] * t.elem_bytes) % 16:
                continue                     # LDS-DMA staging needs rows of 16-byte vectors: refused on this grid whatever the shape
            extra = list(MODE_OPTS[mode])
            if mode in TRIPLE:
                extra += mode_triple(rnd, ndim, [d >= 3 * h * v[0] for d in shape])
            opts = (["--3d"] if ndim == 3 else []) + ["--dtype", dtype] + cl + extra
            if not emulated and not t.registerFilter(opts + [path]):
                continue
            job = ("%s_%s_%s_s%d" % (name, mode, dtype, v[0]), ndim, path, tuple(dims), dtype, opts, v[0])
            break
        assert job, (name, mode)
        jobs.append(job)
    return jobs


def build_args(mode):
    return [j[5] + [j[2]] for j in sample_jobs(mode)]


# the generator's refusals a random configuration of a random shape may meet (the reference refuses the first two alike)
KNOWN_REFUSALS = ("No data to reuse", "Invalid configuration", "KiB of LDS", "--stage dma needs 16-byte vectors")
# ... and the runtime's, decided from the compiler's resource report when build() compiled the kernel: a spill, or no report to read
RUNTIME_REFUSALS = ("exceeds the register file", "no compiler resource report")


def asymmetric_reflecting_axes(pts, ndim, opts):
    """DESIGN section 7's rule: the letters ("z", "y", "x") of the reflecting axes along which the one-step stencil is not its own
    mirror image (a later line of a duplicate offset would replace the earlier one, as in the generator; the committed sample has none)."""
    from boundary_cases import modes_of
    coef = {}
    for p in pts:
        coef[tuple(p[:ndim])] = p[-1]
    out = []
    for ax, (letter, m) in enumerate(zip("zyx"[3 - ndim:], modes_of(list(opts) + ["x"], ndim))):
        if m != "reflect":
            continue
        mirror = {off[:ax] + (-off[ax],) + off[ax + 1:]: c for off, c in coef.items()}
        if mirror != coef:
            out.append(letter)
    return out


if __name__ == "__main__":
    for d in draw_shapes():
        print("shape_%02d_%dd_o%d" % d[:3], d[4], "%d points" % len(d[3]), traits(d[3], d[1]))
