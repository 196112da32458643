#!/usr/bin/env python3
"""Randomised parity sweep on the GPU: random configurations from the tuner's space (all steps, temporal
or fused, odd lane counts, both dtypes) on small ragged grids, each compared with the CPU oracle --
bit for bit for single-pass kernels, within the dtype's bar for temporal pipelines.
--mode periodic | order2 | order2_periodic (or FUZZ_MODE) draws the same space with --boundary periodic and / or --time-order 2 and
checks against the oracle with the host wrap in front of every launch / followed by the subtraction of the old output.
--mode reflect | mixed | source | order2_source: --boundary reflect, a seeded per-axis boundary triple, --source, --time-order 2
--source, against boundary_cases.oracle_boundary_run / source_cases.host_run (tests/options_reference.py).
Builds everything before HIP is initialised."""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tests/ may use the oracle as the checker
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import drstencil_amd as drs
import oracle
from drstencil_amd.tuner import tuning as t
from concurrent.futures import ProcessPoolExecutor

ROUND3 = os.environ.get("FUZZ_ROUND3", "1") != "0"      # 0: the round-2 sweep (same seeds, same configurations as then)
STCS = [(3, "t3_star", 1), (3, "t3_cross", 1), (3, "t3_odd", 1), (2, "t2_star", 1), (2, "t2_box25", 2), (2, "t2_box9", 1), (2, "t2_star9", 2)]

def build(job):
    try:
        drs.Kernel(job[3]); return None
    except Exception as e:
        return "%s: %s" % (" ".join(job[3]), " ".join(str(e).split())[:260])

def round3_knobs(rnd, cl):
    """Round 3's emission knobs, drawn AFTER everything else (the earlier draws of a seed stay what they were): --order rows with
    --pack / --row-fence / --rot-mod, --pin on the taps order, and loader wavefronts behind --stage dma."""
    reuse = "--schedule" not in cl                  # cfgToCommandLine spells scatter out; an explicit --dist alone selects the reuse schedule
    dma = "--stage" in cl
    cyc = "--cyclic-merge-y" in cl and cl[cl.index("--cyclic-merge-y") + 1] != "1"
    r = rnd.random()
    if r < 0.4 and not reuse and not dma and not cyc:
        cl += ["--order", "rows"]
        if rnd.random() < 0.5:
            cl += ["--pack", "0"]
        if rnd.random() < 0.25:
            cl += ["--row-fence", "-1"]
        if rnd.random() < 0.3:
            cl += ["--pin", "0"]
    elif r < 0.6:
        cl += ["--pin", "1"]
    if rnd.random() < 0.3 and not reuse:
        cl += ["--rot-mod", str(rnd.choice([4, 6, 8, 9, 12]))]
    if dma and not reuse and "--defer-stores" not in cl and rnd.random() < 0.6:
        cl += ["--loader-waves", str(rnd.choice([1, 2, 3]))]
        if "--prefetch-depth" not in cl:
            cl += ["--prefetch-depth", str(rnd.choice([1, 2, 3, 4]))]
    # second half of round 3 (drawn last again): coefficients in registers, non-temporal loads by role, reversed block order of every second
    # launch, a published output-array position -- none of them may change a result
    r = rnd.random()
    if r < 0.15:
        cl += ["--coef", rnd.choice(["sgpr", "vgpr"])]
    if rnd.random() < 0.1 and not dma:
        cl += ["--nt-load", str(rnd.choice([2, 3]))]
    if rnd.random() < 0.1:
        cl += ["--zigzag", "1"]
    if rnd.random() < 0.05:
        cl += ["--out-skew", str(rnd.choice([0, 8, 40]))]
    return cl


def round4_knobs(rnd, cl):
    """Round 4's knobs, drawn after round 3's: the skewed temporal pipeline (--skew 1 | 2: needs --prefetch, register staging), the XCD unit /
    chunk maps, and --cyclic-merge-x as the strided layout (taps order, register staging, wherever the configuration merges points in x)."""
    def setopt(name, value):
        if name in cl:
            cl[cl.index(name) + 1] = value
        else:
            cl.extend([name, value])
    if "--temporal" in cl and "--stage" not in cl and rnd.random() < 0.6:
        setopt("--skew", str(rnd.choice([1, 2])))
        if "--prefetch" not in cl:
            cl.append("--prefetch")
    r = rnd.random()
    if r < 0.2:
        setopt("--xcd-remap", "4")
    elif r < 0.35:
        setopt("--xcd-remap", "5")
        setopt("--xcd-chunk", str(rnd.choice([2, 3, 8])))
    if rnd.random() < 0.2 and "--block-merge-x" in cl and "--order" not in cl and "--stage" not in cl:
        cl[cl.index("--block-merge-x")] = "--cyclic-merge-x"
    return cl


MODES = ("fixed", "periodic", "order2", "order2_periodic", "reflect", "mixed", "source", "order2_source")
# the new problem modes draw over the small specs of the periodic and order-2 suites: (ndim, spec, order)
MODE_STCS = [(3, "t3_star", 1), (3, "t3_star_odd", 1), (3, "t3_cross", 1), (3, "t3_odd", 1), (3, "t3_wave", 1),
             (2, "t2_star", 1), (2, "t2_box25", 2), (2, "t2_odd", 1), (2, "t2_wave", 1)]
MODE_OPTS = {"fixed": [], "periodic": ["--boundary", "periodic"], "order2": ["--time-order", "2"],
             "order2_periodic": ["--time-order", "2", "--boundary", "periodic"],
             "reflect": ["--boundary", "reflect"], "mixed": [],         # mixed: a per-axis triple drawn per job (boundary_cases.mode_triple)
             "source": ["--source"], "order2_source": ["--time-order", "2", "--source"]}
STEP1_MODES = ("order2", "order2_periodic", "source", "order2_source")      # what the generator accepts there: step 1, no on-chip stages
MODE = os.environ.get("FUZZ_MODE", "fixed")             # the manual sweeps' mode (fuzz_parity.py / fuzz_shapes.py; --mode on the command line wins)


def job_mode(args):
    """The problem mode a job's argument list names.  --source jobs are "source" / "order2_source" whatever their boundaries (their
    reference takes the per-axis modes from the arguments), every other job with a reflecting or per-axis boundary "reflect" / "mixed"."""
    per = "--boundary" in args and args[args.index("--boundary") + 1] == "periodic"
    o2 = "--time-order" in args and args[args.index("--time-order") + 1] == "2"
    if "--source" in args:
        return "order2_source" if o2 else "source"
    if any(a in args for a in ("--boundary-x", "--boundary-y", "--boundary-z")):
        return "mixed"
    if "--boundary" in args and args[args.index("--boundary") + 1] == "reflect":
        return "reflect"
    return "order2_periodic" if per and o2 else "order2" if o2 else "periodic" if per else "fixed"


def mode_from_argv(argv):
    """--mode <m> taken out of argv (default: FUZZ_MODE, else fixed)."""
    mode = MODE
    if "--mode" in argv:
        i = argv.index("--mode")
        mode = argv[i + 1]
        del argv[i:i + 2]
    if mode not in MODES:
        sys.exit("mode must be one of " + ", ".join(MODES))
    return mode


def make_jobs(n, seed, mode="fixed"):
    """n random configurations (tuner space x test stencils x dtypes): (ndim, stc, dtype, drstencil args, step).  mode "fixed" is the
    sweep as it always was (the module-level generator seeded with `seed`: same draws, same jobs, same kernel cache keys).  The other
    modes draw from a generator of their own over MODE_STCS, n spread evenly over the spec x dtype pairs, append the mode's options and
    skip draws that the tuner's spill model predicts to be refused for scratch;
    the order-2 modes keep to what the generator accepts (step 1, no on-chip stages)."""
    assert mode in MODES, mode
    if mode == "fixed":
        random.seed(seed)
        rnd, stcs = random, STCS
    else:
        rnd, stcs = random.Random("%s/%d" % (mode, seed)), MODE_STCS
    order2 = mode in STEP1_MODES
    jobs = []
    pair = 0
    for ndim, name, order in stcs:
        stc = os.path.join(ROOT, "tests", "stc", name + ".stc")
        for dtype in ("fp32", "fp64"):
            t.order, t.ndim, t.elem_bytes = order, ndim, 4 if dtype == "fp32" else 8
            # FUZZ_STEPS="3,4" FUZZ_SPACE_R4=1: the deep pipelines of round 4 (4 on-chip stages; 11-row workgroups, 36 / 68-lane rows, sn 128 / 256)
            steps = tuple(int(x) for x in os.environ.get("FUZZ_STEPS", "1,2,3").split(","))
            if order2:
                steps = (1,)
            space = t.enumerate_space(steps if order == 1 else tuple(x for x in steps if x <= 2) or (2,), round4=bool(os.environ.get("FUZZ_SPACE_R4")))
            if mode == "fixed":
                count = max(1, n // (2 * len(stcs)))
            else:
                count = n // (2 * len(stcs)) + (pair < n % (2 * len(stcs)))
                pair += 1
            # the new modes oversample and drop what the tuner's spill model predicts the runtime would refuse (tuning.registerFilter, as
            # tests/fuzz_shapes.py does), so that the compiled sample is mostly checked; the fixed sweep compiles every draw, as it always did
            taken = 0
            for v in rnd.sample(space, min(len(space), count if mode == "fixed" else 8 * count)):
                if taken == count:
                    break
                cl = t.cfgToCommandLine(v).split()
                if "cross" in name:
                    i = cl.index("--dist"); cl[i + 1] = str(2 * v[0])
                if ndim == 2 and rnd.random() < 0.5:
                    cl.append("--streaming")
                if "--prefetch-depth" in cl:
                    cl[cl.index("--prefetch-depth") + 1] = str(rnd.choice([1, 2, 3, 4]))
                # round-2 knobs: the reuse schedule's --merge-forward on both sides of the retained planes' tap counts, and the
                # memory path (unconditional / window loads, buffer-masked stores, drains)
                if "--schedule" not in cl and rnd.random() < 0.6:
                    cl[cl.index("--merge-forward") + 1] = str(rnd.choice([0, 2, 3, 100]))
                if rnd.random() < 0.3:
                    cl += ["--uniform-loads", str(rnd.choice([1, 2]))]
                if rnd.random() < 0.3:
                    cl += ["--store-mask", "buffer"]
                if rnd.random() < 0.2:
                    cl += ["--drain", str(rnd.choice([1, 2]))]
                if rnd.random() < 0.3 and "--temporal" not in cl and "--cyclic-merge-y" not in cl and (ndim == 3 or "--streaming" in cl):
                    cl += ["--stage", "dma"]
                if rnd.random() < 0.3:
                    cl += ["--defer-stores", "1"]
                if ROUND3:
                    round3_knobs(rnd, cl)
                    if os.environ.get("FUZZ_ROUND4", "1") != "0":
                        round4_knobs(rnd, cl)
                        if "--skew" in cl and ndim == 2 and "--streaming" not in cl:
                            del cl[cl.index("--skew"):cl.index("--skew") + 2]          # one-shot 2D tiles have no stream to skew
                extra = MODE_OPTS[mode]
                if mode == "mixed":                # drawn last: the earlier draws of a job are those of the other modes' generators
                    import boundary_cases
                    spec = oracle.Spec(stc, ndim, v[0])
                    extra = boundary_cases.mode_triple(rnd, ndim, [d >= 3 * spec.halo for d in spec.shape])
                args = (["--3d"] if ndim == 3 else []) + ["--dtype", dtype] + cl + extra + [stc]
                if mode != "fixed" and not t.registerFilter(args):
                    continue
                taken += 1
                jobs.append((ndim, stc, dtype, args, v[0]))
    return jobs


def signed_random(shape, dtype, seed):
    """Uniform in [-1, 1): both signs, so that sums and the order-2 subtraction cancel."""
    return (np.random.default_rng(seed).random(shape) * 2.0 - 1.0).astype(dtype)


def mode_inputs(spec, dtype, temporal):
    """(A0, B0) of a run in one of the new modes: random A AND random B in [-1, 1) -- with B = 0 the first order-2 launch cannot tell
    -out_old from nothing, and a periodic launch must not read what B's ring holds.  On-chip temporal pipelines (periodic mode only) are
    held to a RELATIVE bar, which means nothing where a sum cancels to nearly zero (one cell in a million is six digits down), so
    they keep non-negative data, [0, 1), like every other temporal case of the project."""
    npdt = np.float32 if dtype == "fp32" else np.float64
    if temporal:
        return np.random.default_rng(11).random(spec.shape).astype(npdt), np.random.default_rng(12).random(spec.shape).astype(npdt)
    return signed_random(spec.shape, npdt, 11), signed_random(spec.shape, npdt, 12)


def mode_reference(spec, A, B, launches, mode):
    """The host reference of `launches` launches of the ping-pong loop in `mode`, in place: the oracle's contracted sweep (fixed),
    with the host wrap in front of every launch (periodic_cases.oracle_periodic_run), or followed by one subtraction of the old output
    (wave_cases.host_run, with the wrap where the mode is periodic too).  The modes whose reference needs the job's own options (a
    per-axis triple, a source array) go through tests/options_reference.py."""
    import periodic_cases, wave_cases
    assert mode in ("fixed", "periodic", "order2", "order2_periodic"), mode
    if mode.startswith("order2"):
        return wave_cases.host_run(spec, A, B, launches, periodic=mode == "order2_periodic")
    if mode == "periodic":
        return periodic_cases.oracle_periodic_run(spec, A, B, launches)
    for i in range(launches):
        src, dst = (A, B) if i % 2 == 0 else (B, A)
        oracle.sweep(spec, src, dst, contract=1)
    return launches


def ring_mask(shape, h):
    ring = np.ones(shape, bool)
    ring[tuple(slice(h, s - h) for s in shape)] = False
    return ring


def rel_error(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)))


def compare_mode_run(spec, mode, dtype, A0, B0, A, B, Ar, Br, launches, temporal):
    """(ok, rel): the arrays a run left against the reference's.  Single-pass kernels (and every gold kernel): both arrays bit for
    bit, which covers the rings -- unchanged under a fixed boundary, the host wrap of the interior under a periodic one.  Temporal
    periodic pipelines: within 1e-6 (fp32) / 1e-12 (fp64) everywhere, and the ring rule: B, wrapped by the last launch and not
    written since, is its own host wrap bit for bit; A's ring is exact after two launches (filled from A0's interior) and the wrap of
    values that are themselves within the bar after more."""
    h = spec.halo
    ring = ring_mask(A0.shape, h)
    if mode in ("fixed", "order2") and not (np.array_equal(A[ring], A0[ring]) and np.array_equal(B[ring], B0[ring])):
        return False, 0.0
    if not temporal:
        return bool(np.array_equal(A, Ar) and np.array_equal(B, Br)), 0.0
    import periodic_cases
    rel = max(rel_error(A, Ar), rel_error(B, Br))
    ring_ok = np.array_equal(B, periodic_cases.host_wrap(B.copy(), h)) and (launches != 2 or np.array_equal(A[ring], Ar[ring]))
    return bool(rel <= (1e-6 if dtype == "fp32" else 1e-12) and ring_ok), rel


def check_mode(job, k, torch, mode):
    """check() for the periodic / order-2 modes: Kernel.run for the spec's iterations from random A and random B against
    mode_reference, then the gold kernel from the same inputs against the same reference (always bit for bit).  The reflect / mixed /
    source / order2_source modes go through options_reference.check_options."""
    if mode in ("reflect", "mixed", "source", "order2_source"):
        from options_reference import check_options
        return check_options(job, k, torch)
    ndim, stc, dtype, args, step = job
    temporal = k.info.get("stages", 1) > 1
    assert not (temporal and mode != "periodic"), "an order-2 kernel with on-chip stages"
    assert k.periodic == mode.endswith("periodic") and k.time_order == (2 if mode.startswith("order2") else 1)
    spec = oracle.Spec(stc, ndim, step)
    A0, B0 = mode_inputs(spec, dtype, temporal)
    Ar, Br = A0.copy(), B0.copy()
    launches = mode_reference(spec, Ar, Br, spec.launches, mode)
    status, worst = "ok", 0.0
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        n = k.run(dA.data_ptr(), dB.data_ptr(), gold=gold)
        torch.cuda.synchronize()
        ok, rel = compare_mode_run(spec, mode, dtype, A0, B0, dA.cpu().numpy(), dB.cpu().numpy(), Ar, Br, launches, temporal and not gold)
        worst = max(worst, rel)
        if n != launches or not ok:
            status = "bad"
    return status, temporal, worst


def check(job, k, torch):
    """One configuration on the GPU against the oracle: ("ok" | "drift" | "bad", temporal, max relative error).  Jobs of the
    periodic / order-2 modes (the mode is read off the job's arguments) go through check_mode."""
    mode = job_mode(job[3])
    if mode != "fixed":
        return check_mode(job, k, torch, mode)
    ndim, stc, dtype, args, step = job
    temporal = k.info.get("stages", 1) > 1
    spec = oracle.Spec(stc, ndim, step)
    A0 = oracle.fill_random(spec.shape, np.float32 if dtype == "fp32" else np.float64)
    Ar, Br = A0.copy(), np.zeros_like(A0)
    oracle.run(spec, Ar, Br, contract=1)
    dA = torch.from_numpy(A0).cuda(); dB = torch.zeros_like(dA)
    k.run(dA.data_ptr(), dB.data_ptr())
    torch.cuda.synchronize()
    A, B = dA.cpu().numpy(), dB.cpu().numpy()
    if temporal:
        rel = max(oracle.check(spec, A, Ar)["max_rel"], oracle.check(spec, B, Br)["max_rel"])
        h = spec.halo
        ring = np.ones(A.shape, bool); ring[tuple(slice(h, s - h) for s in A.shape)] = False
        bar = 1e-6 if dtype == "fp32" else 1e-12
        ring_ok = np.array_equal(A[ring], Ar[ring]) and np.array_equal(B[ring], Br[ring])
        # A temporal pipeline that the generator emitted on its own (--temporal 1) CLAIMS the bar: beyond it is a failure like any
        # other mismatch (the generator's drift estimate, planner.hpp: temporal_drift_per_launch, was wrong).  "drift" exists only for
        # --temporal force kernels: beyond the bar but within 10x of it (and the ring untouched) is the rounding of the
        # intermediate planes the caller asked to see, counted and reported separately, never as a pass
        forced = bool(k.info.get("temporal_forced"))
        return ("ok" if rel <= bar and ring_ok else "drift" if forced and rel <= 10 * bar and ring_ok else "bad"), True, rel
    return ("ok" if np.array_equal(A, Ar) and np.array_equal(B, Br) else "bad"), False, 0.0


def main():
    mode = mode_from_argv(sys.argv)                   # fuzz_parity.py [--mode periodic | order2 | order2_periodic | reflect | mixed | source | order2_source] <n> <seed>
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    jobs = make_jobs(n, int(sys.argv[2]) if len(sys.argv) > 2 else 1, mode)
    t0 = time.time()
    with ProcessPoolExecutor(max_workers=int(os.environ.get("FUZZ_JOBS", "16"))) as ex:
        errs = list(ex.map(build, jobs))
    ok_jobs = [j for j, e in zip(jobs, errs) if e is None]
    rejected = [e for e in errs if e is not None]
    print("built %d kernels in %.0f s; %d configurations rejected by the generator or refused by the runtime (%d for scratch spills)"
          % (len(ok_jobs), time.time() - t0, len(rejected), sum(1 for e in rejected if "scratch" in e)), flush=True)
    for e in rejected[:5]:
        print("  rejected:", e)
    if os.environ.get("FUZZ_BUILD_ONLY"):   # fill the kernel cache on a box without a GPU; the GPU run then finds every kernel built
        return
    kerns = [(j, drs.Kernel(j[3])) for j in ok_jobs]
    import torch
    bad = drift = 0
    worst = {"fp32": 0.0, "fp64": 0.0}
    exact = 0
    for cnt, (job, k) in enumerate(kerns, 1):
        if cnt % 100 == 0:
            print("... %d / %d checked, %d mismatches" % (cnt, len(kerns), bad), flush=True)
        status, temporal, rel = check(job, k, torch)
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
