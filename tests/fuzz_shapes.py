#!/usr/bin/env python3
"""Randomised parity sweep over stencil SHAPES: random point sets inside the order cube (sparse to dense, asymmetric, with or
without the centre, duplicate offsets -- the last one wins, drstencil.hpp:52-78 --, mixed-sign coefficients), 2D and 3D,
orders 1-3, on small ragged grids, each with a few random configurations from the tuner's space (all schedules, every legal
and some illegal --dist) and compared with the CPU oracle like tests/fuzz_parity.py: bit for bit for single-pass kernels,
within the dtype's bar for temporal pipelines.  The hand-written test stencils are stars, boxes and crosses; this sweep is
for everything else the .stc format can say.
usage: fuzz_shapes.py [--mode periodic | order2 | order2_periodic | reflect | mixed | source | order2_source] <shapes> <configurations per shape and dtype> <seed>.
FUZZ_BUILD_ONLY=1 fills the kernel cache on a box without a GPU (the .stc files are regenerated from the seed on either side).
--mode (or FUZZ_MODE) adds --boundary periodic and / or --time-order 2 to every configuration (fuzz_parity.check then compares with
the mode's host reference): periodic configurations whose grid is smaller than 3 Halo of the drawn step in some dimension are skipped
(the generator would reject them: a legal refusal, not a finding), order 2 keeps to step 1 without on-chip stages.  --mode reflect
(--boundary reflect, skipped on small grids like periodic), mixed (a seeded per-axis triple; axes shorter than 3 Halo stay fixed), source
and order2_source (--source, step 1 like order 2) likewise.  The fixed sample of shapes x modes that the test suite runs is
tests/shape_mode_cases.py."""
import itertools, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tests/ may use the oracle as the checker
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import drstencil_amd as drs
from drstencil_amd.tuner import tuning as t
from helpers import write_stc
from concurrent.futures import ProcessPoolExecutor
import fuzz_parity as fp
from shape_knobs import config_options, legal_dists      # shared with the suite's fixed sample (tests/shape_mode_cases.py)

BIG = bool(os.environ.get("FUZZ_SHAPES_BIG"))
dropped = [0]         # configurations the tuner's spill model kept from the compiler
skipped_small = [0]   # periodic configurations on grids smaller than 3 Halo of their step
MAX_TAPS = int(os.environ.get("FUZZ_MAX_TAPS", "420"))        # fused point count above which a step is not tried (compile time)


def random_shape(rnd, ndim, h):
    """(points, mixed_sign): a random subset of [-h, h]^ndim that contains a point at +h along the outermost dimension (the
    reference takes Halo from there, drstencil.hpp:182-196, and every other offset must stay within it)."""
    cells = list(itertools.product(range(-h, h + 1), repeat=ndim))
    density = rnd.choice([0.12, 0.25, 0.5, 0.8, 1.0])
    chosen = [c for c in cells if rnd.random() < density]
    top = tuple([h] + [rnd.randint(-h, h) if rnd.random() < 0.3 else 0 for _ in range(ndim - 1)])
    if not any(c[0] == h for c in chosen):
        chosen.append(top)
    if rnd.random() < 0.3:      # one-sided along the streamed dimension
        chosen = [c for c in chosen if c[0] >= 0] or [top]
    rnd.shuffle(chosen)
    mixed = rnd.random() < 0.25
    if not mixed and rnd.random() < 0.45:
        # two-decimal coefficients: products of up to three of them have six decimals, so rounding the fused coefficients is a
        # no-op and --temporal 1 really emits on-chip stages (planner.hpp falls back to the fused kernel otherwise)
        unit = max(1, int(90 / len(chosen)))
        pts = [c + (rnd.randint(1, unit) / 100.0,) for c in chosen]
    else:
        w = [rnd.uniform(0.02, 1.0) for _ in chosen]
        scale = rnd.uniform(0.7, 1.0) / sum(w)
        pts = [c + ((-1.0 if mixed and rnd.random() < 0.3 else 1.0) * x * scale,) for c, x in zip(chosen, w)]
    if rnd.random() < 0.2:      # a duplicate offset: the later line replaces the earlier one
        c = rnd.choice(pts)
        pts.append(c[:-1] + (c[-1] * 0.5,))
    return pts, mixed


def make_jobs(nshapes, per, seed, mode="fixed"):
    assert mode in fp.MODES and not (BIG and mode != "fixed"), mode      # check_gold knows the fixed boundary only
    rnd = random.Random(seed)
    out = os.path.join(ROOT, "gpurun_out", "fuzz_shapes"); os.makedirs(out, exist_ok=True)
    jobs = []
    for s in range(nshapes):
        ndim = rnd.choice([2, 3])
        h = rnd.choice([1, 1, 2] if ndim == 3 else [1, 2, 2, 3])
        pts, mixed = random_shape(rnd, ndim, h)
        dims = (rnd.randint(18 + 2 * h, 40), rnd.randint(30, 70), rnd.randint(130, 300)) if ndim == 3 else (1, rnd.randint(90, 260), rnd.randint(200, 600))
        if rnd.random() < 0.25:     # grids barely larger than the ring of a 3-step kernel, narrower than a tile, a vector or a wavefront's row
            lo = 6 * h + 1
            dims = (rnd.randint(lo, lo + 5), rnd.randint(lo, lo + 9), rnd.randint(lo, 48)) if ndim == 3 else (1, rnd.randint(lo, lo + 9), rnd.randint(lo, 70))
        if BIG:                     # BASELINE-sized grids: offsets beyond 2^31 bytes, thousands of tiles; checked against the gold kernel
            dims = (rnd.choice([700, 1024]), rnd.choice([1000, 1024]), rnd.choice([1024, 1100])) if ndim == 3 else (1, rnd.choice([8192, 12000]), rnd.choice([8192, 16384]))
        stc = os.path.join(out, "shape%d_s%d_%dd_o%d.stc" % (seed, s, ndim, h))
        write_stc(stc, ndim, dims, rnd.randint(1, 7), pts)     # iterations: 2 * ceil(iterations / (2 * step)) launches (codegen.hpp:581-584)
        distinct = len(set(p[:-1] for p in pts))
        steps = tuple(st for st in (1, 2, 3) if min((2 * h * st + 1) ** ndim, distinct ** st) <= MAX_TAPS)
        if mode in fp.STEP1_MODES:
            steps = (1,)                         # what the generator accepts with --time-order 2 (no --temporal at step 1 either)
        dists = {}
        for dtype in ("fp32", "fp64"):
            t.order, t.ndim, t.elem_bytes = h, ndim, 4 if dtype == "fp32" else 8
            space = t.enumerate_space(steps)
            for v in rnd.sample(space, min(len(space), per)):
                cl = config_options(rnd, v, ndim, h, pts, mixed, dists)
                if cl is None:
                    continue
                if (mode.endswith("periodic") or mode == "reflect") and min(dims[3 - ndim:]) < 3 * h * v[0]:
                    skipped_small[0] += 1        # --boundary periodic | reflect needs every dimension >= 3 Halo (Halo = step * order)
                    continue
                extra = fp.MODE_OPTS[mode]
                if mode == "mixed":              # drawn last
                    import boundary_cases
                    extra = boundary_cases.mode_triple(rnd, ndim, [d >= 3 * h * v[0] for d in dims[3 - ndim:]])
                args = (["--3d"] if ndim == 3 else []) + ["--dtype", dtype] + cl + extra + [stc]
                if not t.registerFilter(args):   # the tuner's spill model: do not compile what would be refused for scratch
                    dropped[0] += 1
                    continue
                jobs.append((ndim, stc, dtype, args, v[0]))
    return jobs


def check_gold(job, k, torch):
    """FUZZ_SHAPES_BIG: the optimised kernel against the gold kernel of the same emitted source (the oracle would take minutes
    per configuration at these sizes; the gold kernel's arithmetic is pinned to it on the small grids)."""
    ndim, stc, dtype, args, step = job
    info = k.info
    shape = (info["L"], info["M"], info["N"]) if ndim == 3 else (info["M"], info["N"])
    tdt = torch.float32 if dtype == "fp32" else torch.float64
    g = torch.Generator(device="cuda").manual_seed(7)
    A0 = torch.rand(shape, dtype=tdt, device="cuda", generator=g)
    A, B, Ag, Bg = A0.clone(), torch.zeros_like(A0), A0.clone(), torch.zeros_like(A0)
    k.run(A.data_ptr(), B.data_ptr())
    k.run(Ag.data_ptr(), Bg.data_ptr(), gold=True)
    torch.cuda.synchronize()
    if info.get("stages", 1) > 1:
        h = info["halo"]
        inner = tuple(slice(h, n - h) for n in shape)
        rel = max(float(((X - G)[inner].abs() / G[inner].abs().clamp_min(1e-30)).max()) for X, G in ((A, Ag), (B, Bg)))
        ring_ok = True
        for X, G in ((A, Ag), (B, Bg)):
            D = X != G
            D[inner] = False
            ring_ok = ring_ok and not bool(D.any())
        bar = 1e-6 if dtype == "fp32" else 1e-12
        forced = bool(info.get("temporal_forced"))       # only --temporal force kernels may drift (fuzz_parity.check)
        return ("ok" if rel <= bar and ring_ok else "drift" if forced and rel <= 10 * bar and ring_ok else "bad"), True, rel
    return ("ok" if torch.equal(A, Ag) and torch.equal(B, Bg) else "bad"), False, 0.0


def main():
    mode = fp.mode_from_argv(sys.argv)
    nshapes = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    jobs = make_jobs(nshapes, per, int(sys.argv[3]) if len(sys.argv) > 3 else 1, mode)
    if skipped_small[0]:
        print("%d periodic / reflecting configurations skipped: grid smaller than 3 Halo of the drawn step" % skipped_small[0])
    t0 = time.time()
    with ProcessPoolExecutor(max_workers=int(os.environ.get("FUZZ_JOBS", "16"))) as ex:
        errs = list(ex.map(fp.build, jobs, chunksize=4))
    ok_jobs = [j for j, e in zip(jobs, errs) if e is None]
    rejected = [e for e in errs if e is not None]
    why = {}
    for e in rejected:
        msg = e.split(": ", 1)[1] if ": " in e else e
        key = "scratch spills" if "scratch" in msg else " ".join(msg.split()[:9])
        why[key] = why.get(key, 0) + 1
    print("%d shapes, %d configurations (+%d dropped by the tuner's spill model): built %d kernels in %.0f s; %d rejected by the generator or refused by the runtime"
          % (nshapes, len(jobs), dropped[0], len(ok_jobs), time.time() - t0, len(rejected)), flush=True)
    for k, n in sorted(why.items(), key=lambda kv: -kv[1])[:12]:
        print("  %5d x %s" % (n, k))
    if os.environ.get("FUZZ_BUILD_ONLY"):
        return
    kerns = [(j, drs.Kernel(j[3])) for j in ok_jobs]
    import torch
    bad = exact = drift = 0
    worst = {"fp32": 0.0, "fp64": 0.0}
    for cnt, (job, k) in enumerate(kerns, 1):
        if cnt % 100 == 0:
            print("... %d / %d checked, %d mismatches" % (cnt, len(kerns), bad), flush=True)
        status, temporal, rel = check_gold(job, k, torch) if BIG else fp.check(job, k, torch)
        if temporal:
            worst[job[2]] = max(worst[job[2]], rel)
        else:
            exact += status == "ok"
        if status == "drift":
            drift += 1
            print("DRIFT (temporal pipeline beyond the bar, rel %.3g)" % rel, " ".join(job[3][:-1]), os.path.basename(job[1]), flush=True)
        elif status != "ok":
            bad += 1
            print("MISMATCH", " ".join(job[3][:-1]), os.path.basename(job[1]), "rel %.3g" % rel, flush=True)
    print("%d configurations checked: %d single-pass bit-exact, %d temporal within tolerance (worst fp32 %.3g, fp64 %.3g), %d temporal beyond 1e-6 / 1e-12 by rounding drift, %d MISMATCHES"
          % (len(kerns), exact, len(kerns) - exact - bad - drift, worst["fp32"], worst["fp64"], drift, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
