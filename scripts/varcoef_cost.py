"""What --varcoef costs: the tuned step-1 kernel (out = S(in)), the same kernel at the geometry the --varcoef fit rule steps down to, and
that geometry with --varcoef (out = sum_t a_t * in[. + d_t]), timed on one GPU with HIP events, alternating in one run, several repeats
each.

    python scripts/varcoef_cost.py --out profiles/varcoef_cost.json        # C2 and C4, tuned step-1 rows

By bytes a --varcoef launch moves 2 + T arrays where the step-1 launch moves 2, so its yardstick is the plain kernel OF THE SAME RUN
times (2 + T) / 2; the plain kernel at the stepped-down geometry tells the step-down from the streams.  There is no pass bar: the script
reports the ratios and the plain kernel's run-to-run spread.  Every timed loop starts from the same finite data (uniform in [0, 1), the
coefficients in [0.5, 1) / T), all variants share one arena -- the pair at the step-1 kernel's recommended placement, the T coefficient
grids behind it -- and every timed kernel is verified once against its gold kernel.  The kernels are the ones tests/varcoef_cases.py
lists (prebuilt by __graft_entry__.build()); nothing here runs hipcc."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MIN_WARM_S = 1.0
HBM_PEAK = 8e12
NAMES = ("plain", "plain_stepped_down", "varcoef")


def measure(args):
    import torch
    import drstencil_amd as drs
    import bench
    from varcoef_cases import cost_cases
    os.environ["DRS_NO_COMPILE"] = "1"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rows = []
    for w, *opts in cost_cases():
        if args.only and w not in args.only:
            continue
        wl = bench.WORKLOADS[w]
        kern, refused = {}, {}
        for name, o in zip(NAMES, opts):
            try:
                kern[name] = drs.Kernel(o + [wl["stc"]])
            except drs.KernelBuildError as e:          # the runtime refuses a kernel that spills: reported, not timed
                refused[name] = " ".join(str(e).split())[:400]
        assert "plain" in kern and not kern["plain"].varcoef
        i = kern["plain"].info
        T = i["taps"]
        arrays = {"plain": 2, "plain_stepped_down": 2, "varcoef": 2 + T}
        tdt = torch.float32 if i["dtype"] == "fp32" else torch.float64
        esz = 4 if i["dtype"] == "fp32" else 8
        shape = (i["L"], i["M"], i["N"]) if i["ndim"] == 3 else (i["M"], i["N"])
        g = torch.Generator(device=dev).manual_seed(1)
        A0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        B0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        # one arena: the pair laid out by the step-1 kernel's pair_layout(), the coefficient grids behind it at the next 256-byte boundary
        pair_bytes, b_off = kern["plain"].pair_layout()
        nb = kern["plain"].array_bytes()
        k_off = -(-pair_bytes // 256) * 256
        arena = torch.empty(k_off + T * nb, dtype=torch.uint8, device=dev)
        A, B = (arena[o:o + nb].view(tdt).view(shape) for o in (0, b_off))
        K = arena[k_off:k_off + T * nb].view(tdt).view((T,) + shape)
        assert B.data_ptr() - A.data_ptr() == b_off and K.data_ptr() - A.data_ptr() == k_off >= b_off + nb and A.numel() == A0.numel()
        for t in range(T):
            K[t].copy_((torch.rand(shape, dtype=tdt, device=dev, generator=g) * 0.5 + 0.5) / T)
        launches = args.launches

        def kw_of(k):
            return {"d_coef": K.data_ptr()} if k.varcoef else {}

        def loop(k):
            A.copy_(A0); B.copy_(B0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            n = k.run(A.data_ptr(), B.data_ptr(), iterations=launches, stream=stream.cuda_stream, **kw_of(k))
            e1.record(stream)
            torch.cuda.synchronize()
            assert n == launches
            return e0.elapsed_time(e1) / n

        Bg = torch.empty_like(A0)
        checks = {}
        for name, k in kern.items():
            A.copy_(A0); B.copy_(B0); Bg.copy_(B0)
            k.launch(A.data_ptr(), B.data_ptr(), **kw_of(k))
            k.launch_gold(A.data_ptr(), Bg.data_ptr(), **kw_of(k))
            torch.cuda.synchronize()
            checks[name] = {"dr_equals_gold": bool(torch.equal(B, Bg)), "finite": bool(torch.isfinite(B).all())}
        del Bg
        for k in kern.values():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < MIN_WARM_S:
                loop(k)
        ms = {name: [] for name in kern}
        order = list(kern)
        for r in range(args.repeats):
            for name in (order if r % 2 == 0 else order[::-1]):
                ms[name].append(loop(kern[name]))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        pts = int(A0.numel())
        spread = (max(ms["plain"]) - min(ms["plain"])) / med["plain"]
        ratios = {k: med[k] / med["plain"] for k in med if k != "plain"}
        row = {"id": w, "workload": wl["name"], "taps": T, "options": {n: " ".join(o) for n, o in zip(NAMES, opts)}, "launches_per_loop": launches, "repeats": args.repeats,
               "resources": {k: {x: kern[k].resources.get(x) for x in ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")} for k in kern},
               "arena": {"array_bytes": nb, "out_offset": b_off, "coef_offset": k_off},
               "refused_by_the_runtime": refused,
               "ms_per_launch": {k: [round(x, 5) for x in v] for k, v in ms.items()},
               "median_ms_per_launch": {k: round(v, 5) for k, v in med.items()},
               "fraction_of_8TBps": {k: round(arrays[k] * esz * pts / (v * 1e-3) / HBM_PEAK, 4) for k, v in med.items()},
               "time_over_plain": {k: round(v, 4) for k, v in ratios.items()},
               "expected_by_bytes": {k: arrays[k] / 2.0 for k in ratios},
               "plain_run_to_run_spread": round(spread, 4),
               "varcoef_over_bytes_yardstick": round(ratios["varcoef"] / (arrays["varcoef"] / 2.0), 4) if "varcoef" in ratios else None,
               "varcoef_over_plain_stepped_down": round(med["varcoef"] / med["plain_stepped_down"], 4) if "varcoef" in med and "plain_stepped_down" in med else None,
               "verified": checks}
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("id", "median_ms_per_launch", "fraction_of_8TBps", "time_over_plain", "expected_by_bytes", "varcoef_over_bytes_yardstick",
                                              "varcoef_over_plain_stepped_down", "plain_run_to_run_spread", "refused_by_the_runtime", "verified")}), flush=True)
        del A, B, K, arena, A0, B0
        torch.cuda.empty_cache()
    res = {"what": "tuned step-1 kernel plain / plain at the --varcoef fit rule's stepped-down geometry / that geometry with --varcoef, one arena (the pair at the "
                   "step-1 kernel's recommended placement, the T coefficient grids behind it), HIP events around run() of launches_per_loop launches, alternating, "
                   "both arrays restored before every loop; median over repeats.  fraction_of_8TBps counts 2 / 2 / (2 + T) x sizeof x grid points per launch",
           "device": torch.cuda.get_device_name(0), "cases": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    ok = all(all(c.values()) for r in rows for c in r["verified"].values())
    print("written %s, verified %s" % (args.out, ok))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="varcoef_cost.json")
    ap.add_argument("--only", nargs="*", help="case ids (c4, c2)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed loop (even)")
    return measure(ap.parse_args())


if __name__ == "__main__":
    sys.exit(main())
