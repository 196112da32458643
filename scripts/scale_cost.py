"""What --scale costs: the tuned step-1 kernel (out = S(in)), the same kernel with --source (out = S(in) + src), with --scale
(out = w * S(in)) and with --scale --scale-centre 1 (out = in + w * S(in)), timed on one GPU with HIP events, alternating in one run,
several repeats each.

    python scripts/scale_cost.py --out profiles/scale_cost.json        # C2 and C4, tuned step-1 rows

By bytes --source and --scale move 3 arrays where the step-1 launch moves 2 (the centre values are re-reads of lines the sweep has just
fetched), so the yardstick of the --scale kernel is the --source kernel of the same tuned row IN THE SAME RUN: the script reports
scale / source, scale_centre / scale and the plain kernel's run-to-run spread, and says where a ratio leaves 1 +- 3 x spread.  There is no
pass bar.  Every timed loop starts from the same finite data (uniform in [0, 1), the source scaled by 1e-3, the factors in [0.25, 0.75)),
all variants share one arena -- the pair at the step-1 kernel's recommended placement, and behind it ONE slot that holds src for the
--source kernel and w for the --scale kernels -- and every timed kernel is verified once against its gold kernel.  The kernels are the
ones tests/scale_cases.py lists (prebuilt by __graft_entry__.build()); nothing here runs hipcc."""
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
NAMES = ("plain", "source", "scale", "scale_centre")
ARRAYS = {"plain": 2, "source": 3, "scale": 3, "scale_centre": 3}


def measure(args):
    import torch
    import drstencil_amd as drs
    import bench
    from scale_cases import cost_cases
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
        assert "plain" in kern and not kern["plain"].source and not kern["plain"].scale
        i = kern["plain"].info
        tdt = torch.float32 if i["dtype"] == "fp32" else torch.float64
        esz = 4 if i["dtype"] == "fp32" else 8
        shape = (i["L"], i["M"], i["N"]) if i["ndim"] == 3 else (i["M"], i["N"])
        g = torch.Generator(device=dev).manual_seed(1)
        A0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        B0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        # one arena: the pair laid out by the step-1 kernel's pair_layout(), the third array's slot behind it at the next 256-byte boundary
        pair_bytes, b_off = kern["plain"].pair_layout()
        nb = kern["plain"].array_bytes()
        f_off = -(-pair_bytes // 256) * 256
        arena = torch.empty(f_off + nb, dtype=torch.uint8, device=dev)
        A, B, F = (arena[o:o + nb].view(tdt).view(shape) for o in (0, b_off, f_off))
        assert B.data_ptr() - A.data_ptr() == b_off and F.data_ptr() - A.data_ptr() == f_off >= b_off + nb and A.numel() == A0.numel()
        F0 = torch.rand(shape, dtype=tdt, device=dev, generator=g) * 1e-3
        W0 = torch.rand(shape, dtype=tdt, device=dev, generator=g) * 0.5 + 0.25
        launches = args.launches

        def third(k):
            """The keyword of the kernel's third array, its slot filled with that kernel's data (outside every timed region)."""
            if k.source:
                F.copy_(F0)
                return {"d_src": F.data_ptr()}
            if k.scale:
                F.copy_(W0)
                return {"d_scale": F.data_ptr()}
            return {}

        def loop(k):
            A.copy_(A0); B.copy_(B0)
            kw = third(k)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            n = k.run(A.data_ptr(), B.data_ptr(), iterations=launches, stream=stream.cuda_stream, **kw)
            e1.record(stream)
            torch.cuda.synchronize()
            assert n == launches
            return e0.elapsed_time(e1) / n

        Bg = torch.empty_like(A0)
        checks = {}
        for name, k in kern.items():
            A.copy_(A0); B.copy_(B0); Bg.copy_(B0)
            kw = third(k)
            k.launch(A.data_ptr(), B.data_ptr(), **kw)
            k.launch_gold(A.data_ptr(), Bg.data_ptr(), **kw)
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
        row = {"id": w, "workload": wl["name"], "options": " ".join(opts[0]), "launches_per_loop": launches, "repeats": args.repeats,
               "resources": {k: {x: kern[k].resources.get(x) for x in ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")} for k in kern},
               "arena": {"array_bytes": nb, "out_offset": b_off, "src_offset": f_off},
               "refused_by_the_runtime": refused,
               "ms_per_launch": {k: [round(x, 5) for x in v] for k, v in ms.items()},
               "median_ms_per_launch": {k: round(v, 5) for k, v in med.items()},
               "fraction_of_8TBps": {k: round(ARRAYS[k] * esz * pts / (v * 1e-3) / HBM_PEAK, 4) for k, v in med.items()},
               "time_over_plain": {k: round(v, 4) for k, v in ratios.items()},
               "expected_by_bytes": {k: ARRAYS[k] / 2.0 for k in ratios},
               "plain_run_to_run_spread": round(spread, 4),
               "ratio_exceeds_expectation_by_more_than_spread": {k: bool(v > ARRAYS[k] / 2.0 * (1.0 + spread)) for k, v in ratios.items()},
               "scale_over_source": round(med["scale"] / med["source"], 4) if "scale" in med and "source" in med else None,
               "scale_centre_over_scale": round(med["scale_centre"] / med["scale"], 4) if "scale_centre" in med and "scale" in med else None,
               "leaves_1_pm_3_spreads": {n: bool(abs(med[a] / med[b] - 1.0) > 3.0 * spread) for n, a, b in (("scale_over_source", "scale", "source"), ("scale_centre_over_scale", "scale_centre", "scale"))
                                         if a in med and b in med},
               "verified": checks}
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("id", "median_ms_per_launch", "fraction_of_8TBps", "time_over_plain", "scale_over_source", "scale_centre_over_scale", "plain_run_to_run_spread",
                                              "leaves_1_pm_3_spreads", "refused_by_the_runtime", "verified")}), flush=True)
        del A, B, arena, A0, B0, F, F0, W0
        torch.cuda.empty_cache()
    res = {"what": "tuned step-1 kernel plain / with --source / with --scale / with --scale --scale-centre 1, one arena (the pair at the step-1 kernel's recommended placement, "
                   "src or w in one slot behind it), HIP events around run() of launches_per_loop launches, alternating, both arrays restored before "
                   "every loop; median over repeats.  fraction_of_8TBps counts 2 / 3 / 3 / 3 x sizeof x grid points per launch",
           "device": torch.cuda.get_device_name(0), "cases": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    ok = all(all(c.values()) for r in rows for c in r["verified"].values())
    print("written %s, verified %s" % (args.out, ok))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="scale_cost.json")
    ap.add_argument("--only", nargs="*", help="case ids (c4, c2)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed loop (even)")
    return measure(ap.parse_args())


if __name__ == "__main__":
    sys.exit(main())
