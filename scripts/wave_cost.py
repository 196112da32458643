"""What --time-order 2 costs: the tuned step-1 kernel (out = S(in)) and the same kernel with --time-order 2 (out = S(in) - out_old, a third
memory stream), timed on one GPU with HIP events, alternating, several repeats each.

    python scripts/wave_cost.py --out profiles/wave_cost.json            # C4 and C2, tuned step-1 rows
    rocprofv3 --kernel-trace --stats -d TRACE -o c4 -- python scripts/wave_cost.py --only c4 --repeats 2 --skews 0 --out /tmp/x.json

By bytes an order-2 launch moves 3 arrays where the step-1 launch moves 2: the expectation is 1.5 x the step-1 launch time.  Every timed
loop starts from the same finite data in BOTH arrays (the leapfrog recurrence with the shipped coefficients is stable: |symbol| <= 2), all
variants share one arena, and every timed kernel is verified once against its gold kernel.  The output is now read as well, so the
placement (out - in) mod 64 MiB is measured again for the order-2 kernel (--skews, MiB) instead of taken from the step-1 kernel.  The
kernels are the ones tests/wave_cases.py lists (prebuilt by __graft_entry__.build()); nothing here runs hipcc."""
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


def verify(torch, kern, A0, B0, A, B, Bg):
    """One launch from (A0, B0) against the gold kernel, bit for bit on the whole grid."""
    A.copy_(A0); B.copy_(B0); Bg.copy_(B0)
    kern.launch(A.data_ptr(), B.data_ptr())
    kern.launch_gold(A.data_ptr(), Bg.data_ptr())
    torch.cuda.synchronize()
    return {"dr_equals_gold": bool(torch.equal(B, Bg)), "output_changed": not bool(torch.equal(B, B0)), "ok": bool(torch.equal(B, Bg)) and not bool(torch.equal(B, B0))}


def measure(args):
    import torch
    import drstencil_amd as drs
    import bench
    from wave_cases import cost_cases
    os.environ["DRS_NO_COMPILE"] = "1"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rows = []
    for cid, w, first_opts, second_opts in cost_cases():
        if args.only and cid not in args.only:
            continue
        wl = bench.WORKLOADS[w]
        kern = {"order1": drs.Kernel(first_opts + [wl["stc"]]), "order2": drs.Kernel(second_opts + [wl["stc"]])}
        assert kern["order2"].time_order == 2 and kern["order1"].time_order == 1
        i = kern["order1"].info
        tdt = torch.float32 if i["dtype"] == "fp32" else torch.float64
        esz = 4 if i["dtype"] == "fp32" else 8
        shape = (i["L"], i["M"], i["N"]) if i["ndim"] == 3 else (i["M"], i["N"])
        g = torch.Generator(device=dev).manual_seed(1)
        A0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        B0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        launches = args.launches

        def loop(k, A, B):
            A.copy_(A0); B.copy_(B0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            n = k.run(A.data_ptr(), B.data_ptr(), iterations=launches, stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            assert n == launches
            return e0.elapsed_time(e1) / n

        # placement: (out - in) mod 64 MiB, both kernels, the project's own recommendation first
        rec = int(i.get("out_skew_bytes", 0)) >> 20
        skews = [rec] + [s for s in (args.skews if args.skews is not None else [0, 8, 16, 24, 32, 40, 48, 56]) if s != rec]
        placement = {}
        for s in skews:
            A, B, arena = kern["order1"].alloc_pair(torch, dev, dtype=tdt, skew=s << 20)
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < (MIN_WARM_S if s == skews[0] else 0.1):
                loop(kern["order2"], A, B)
            placement[s] = {name: round(min(loop(kern[name], A, B) for _ in range(3)), 5) for name in ("order1", "order2")}
            del A, B, arena
            torch.cuda.empty_cache()
        best = min(placement, key=lambda s: placement[s]["order2"])
        # the comparison proper: one arena at the step-1 kernel's recommended placement (what callers of the C ABI get), alternating
        A, B, arena = kern["order1"].alloc_pair(torch, dev, dtype=tdt, skew=rec << 20)
        Bg = torch.empty_like(A0)
        checks = {name: verify(torch, kern[name], A0, B0, A, B, Bg) for name in kern}
        del Bg
        for name in kern:
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < MIN_WARM_S:
                loop(kern[name], A, B)
        ms = {"order1": [], "order2": []}
        for r in range(args.repeats):
            for name in (("order1", "order2") if r % 2 == 0 else ("order2", "order1")):
                ms[name].append(loop(kern[name], A, B))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        ups = kern["order1"].updates_per_launch()
        pts = int(A0.numel())
        spread1 = (max(ms["order1"]) - min(ms["order1"])) / med["order1"]
        ratio = med["order2"] / med["order1"]
        row = {"id": cid, "workload": wl["name"], "options": " ".join(first_opts), "launches_per_loop": launches, "repeats": args.repeats,
               "resources": {k: {x: kern[k].resources.get(x) for x in ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")} for k in kern},
               "ms_per_launch": {k: [round(x, 5) for x in v] for k, v in ms.items()},
               "median_ms_per_launch": {k: round(v, 5) for k, v in med.items()},
               "gstencil_per_s": {k: round(ups / (v * 1e-3) / 1e9, 2) for k, v in med.items()},
               "fraction_of_8TBps": {"order1": round(2 * esz * pts / (med["order1"] * 1e-3) / HBM_PEAK, 4),
                                     "order2": round(3 * esz * pts / (med["order2"] * 1e-3) / HBM_PEAK, 4)},
               "order2_over_order1_time": round(ratio, 4), "expected_by_bytes": 1.5,
               "order1_run_to_run_spread": round(spread1, 4),
               "ratio_exceeds_1.5_by_more_than_spread": bool(ratio > 1.5 * (1.0 + spread1)),
               "placement_MiB_min_ms_per_launch": {str(s): placement[s] for s in skews},
               "placement_recommended_MiB": rec, "placement_best_for_order2_MiB": best,
               "verified": checks}
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("id", "median_ms_per_launch", "gstencil_per_s", "fraction_of_8TBps", "order2_over_order1_time",
                                              "order1_run_to_run_spread", "placement_best_for_order2_MiB", "verified")}), flush=True)
        del A, B, arena, A0, B0
        torch.cuda.empty_cache()
    res = {"what": "tuned step-1 kernel without / with --time-order 2, same arena (the step-1 kernel's recommended placement), HIP events around "
                   "run() of launches_per_loop launches, alternating, both arrays restored before every loop; median over repeats.  "
                   "fraction_of_8TBps counts 2 (order 1) / 3 (order 2) x sizeof x grid points per launch",
           "device": torch.cuda.get_device_name(0), "cases": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    ok = all(r["verified"][k]["ok"] for r in rows for k in r["verified"])
    print("written %s, verified %s" % (args.out, ok))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="wave_cost.json")
    ap.add_argument("--only", nargs="*", help="case ids (c4, c2)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed loop (even)")
    ap.add_argument("--skews", type=int, nargs="*", help="placements (out - in) mod 64 MiB to measure, in MiB (default: 0 8 ... 56)")
    return measure(ap.parse_args())


if __name__ == "__main__":
    sys.exit(main())
