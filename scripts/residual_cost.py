"""What --residual max costs: a tuned kernel (out = S(in)) and the same kernel with --residual max (the launch also writes
r = max |out - in| over the interior: one more read of `in` at the cells it stores, a per-lane maximum, one partial per workgroup and a
one-workgroup fold kernel behind the sweep), timed on one GPU with HIP events, alternating in one run, several repeats each.

    python scripts/residual_cost.py --out profiles/residual_cost.json        # C2 step 1, C4 step 1, C4 fused step 2
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d PMC -- python scripts/residual_cost.py --only "C4 step 1" --repeats 1 --launches 2 --warm-seconds 0 --out /tmp/x.json
    python scripts/residual_cost.py --fetch-size PMC        # FETCH_SIZE per launch of the counter run: sweeps followed by res_<name> against the others
(the counter run and --fetch-size have not been run on a GPU yet: profiles/residual_cost.json holds the timings only)

By bytes the launch should take between 1.0 x the plain launch (the centre re-read served from L2: the workgroup fetched those lines
a few planes earlier) and 1.5 x (a third array from HBM).  Every timed loop starts from the same finite data (uniform in [0, 1)), both
kernels use one arena -- the pair at the plain kernel's recommended placement, the residual array behind it -- and every timed kernel
is verified once: its arrays against its gold kernel, the residual against torch's max |out - in| over the interior in the array's
dtype.  A row whose --residual kernel the runtime refuses (it spills) is reported as refused, not timed.  The kernels are the ones
tests/residual_cases.py lists (prebuilt by __graft_entry__.build()); nothing here runs hipcc."""
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
KEYS = ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")


def measure(args):
    import torch
    import drstencil_amd as drs
    import bench
    from residual_cases import cost_cases
    os.environ["DRS_NO_COMPILE"] = "1"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rows = []
    for label, w, plain_opts, res_opts in cost_cases():
        if args.only and label not in args.only:
            continue
        wl = bench.WORKLOADS[w]
        kern, refused = {}, {}
        for name, o in (("plain", plain_opts), ("residual", res_opts)):
            try:
                kern[name] = drs.Kernel(o + [wl["stc"]])
            except drs.KernelBuildError as e:          # the runtime refuses a kernel that spills: reported, not timed
                refused[name] = " ".join(str(e).split())[:400]
        assert "plain" in kern and not kern["plain"].residual_elems
        i = kern["plain"].info
        H = i["halo"]
        tdt = torch.float32 if i["dtype"] == "fp32" else torch.float64
        esz = 4 if i["dtype"] == "fp32" else 8
        shape = (i["L"], i["M"], i["N"]) if i["ndim"] == 3 else (i["M"], i["N"])
        inner = tuple(slice(H, n - H) for n in shape)
        g = torch.Generator(device=dev).manual_seed(1)
        A0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        B0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        pair_bytes, b_off = kern["plain"].pair_layout()
        nb = kern["plain"].array_bytes()
        r_off = -(-pair_bytes // 256) * 256
        relems = kern["residual"].residual_elems if "residual" in kern else 1
        arena = torch.empty(r_off + relems * esz, dtype=torch.uint8, device=dev)
        A, B = (arena[o:o + nb].view(tdt).view(shape) for o in (0, b_off))
        R = arena[r_off:r_off + relems * esz].view(tdt)
        launches = args.launches

        def res_of(k):
            return {"d_res": R.data_ptr()} if k.residual_elems else {}

        def loop(k):
            A.copy_(A0); B.copy_(B0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            n = k.run(A.data_ptr(), B.data_ptr(), iterations=launches * i["step"], stream=stream.cuda_stream, **res_of(k))
            e1.record(stream)
            torch.cuda.synchronize()
            assert n == launches, (n, launches)
            return e0.elapsed_time(e1) / n

        Bg = torch.empty_like(A0)
        checks = {}
        for name, k in kern.items():
            A.copy_(A0); B.copy_(B0); Bg.copy_(B0)
            R.fill_(float("nan"))
            k.launch(A.data_ptr(), B.data_ptr(), **res_of(k))
            k.launch_gold(A.data_ptr(), Bg.data_ptr())
            torch.cuda.synchronize()
            checks[name] = {"dr_equals_gold": bool(torch.equal(B, Bg)), "finite": bool(torch.isfinite(B).all())}
            if k.residual_elems:
                want = (Bg[inner] - A[inner]).abs().max()
                checks[name]["residual_equals_max_abs_diff"] = bool(torch.equal(R[0], want))
                checks[name]["every_partial_written"] = bool(not torch.isnan(R).any())
        del Bg
        for k in kern.values():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < args.warm_seconds:
                loop(k)
        ms = {name: [] for name in kern}
        order = list(kern)
        for r in range(args.repeats):
            for name in (order if r % 2 == 0 else order[::-1]):
                ms[name].append(loop(kern[name]))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        pts = int(A0.numel())
        spread = (max(ms["plain"]) - min(ms["plain"])) / med["plain"]
        ratio = med["residual"] / med["plain"] if "residual" in med else None
        row = {"id": label, "workload": wl["name"], "options": " ".join(plain_opts), "launches_per_loop": launches, "repeats": args.repeats,
               "resources": {k: {x: kern[k].resources.get(x) for x in KEYS} for k in kern},
               "reg_demand": {k: kern[k].info["reg_demand"] for k in kern},
               "residual_elems": relems if "residual" in kern else None,
               "arena": {"array_bytes": nb, "out_offset": b_off, "res_offset": r_off},
               "refused_by_the_runtime": refused,
               "ms_per_launch": {k: [round(x, 5) for x in v] for k, v in ms.items()},
               "median_ms_per_launch": {k: round(v, 5) for k, v in med.items()},
               "fraction_of_8TBps_counting_two_arrays": {k: round(2 * esz * pts / (v * 1e-3) / HBM_PEAK, 4) for k, v in med.items()},
               "time_over_plain": None if ratio is None else round(ratio, 4),
               "expected_by_bytes": [1.0, 1.5],
               "plain_run_to_run_spread": round(spread, 4),
               "ratio_exceeds_1_by_more_than_spread": None if ratio is None else bool(ratio > 1.0 + spread),
               "verified": checks}
        rows.append(row)
        print(json.dumps({k: row[k] for k in ("id", "median_ms_per_launch", "time_over_plain", "plain_run_to_run_spread", "resources", "refused_by_the_runtime", "verified")}), flush=True)
        del A, B, R, arena, A0, B0
        torch.cuda.empty_cache()
    res = {"what": "a tuned kernel plain / with --residual max, one arena (the pair at the plain kernel's recommended placement, the residual array behind "
                   "it), HIP events around run() of launches_per_loop launches, alternating, both arrays restored before every loop; median over repeats",
           "device": torch.cuda.get_device_name(0), "cases": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    ok = all(all(c.values()) for r in rows for c in r["verified"].values())
    print("written %s, verified %s" % (args.out, ok))
    return 0 if ok else 1


def fetch_size(root):
    """Per-launch FETCH_SIZE of a counters-only rocprofv3 run of this script: the dr_ dispatches that a res_ dispatch follows are the
    --residual sweeps, the other dr_ dispatches the plain ones (both kernels carry the spec's name).  Pure CSV parsing."""
    import csv
    import glob
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f, errors="replace")):
            if r.get("Counter_Name") == "FETCH_SIZE":
                rows.append((int(r["Dispatch_Id"]), r["Kernel_Name"], float(r["Counter_Value"])))
    rows.sort()
    out = {}
    for n, (d, name, v) in enumerate(rows):
        if not name.startswith("dr_"):
            continue
        kind = "residual" if n + 1 < len(rows) and rows[n + 1][1].startswith("res_") else "plain"
        out.setdefault(name.split("(")[0] + " " + kind, []).append(v)
    res = {k: {"dispatches": len(v), "FETCH_SIZE_per_launch": sum(v) / len(v), "GiB_at_1KiB_units_x2_gfx950": sum(v) / len(v) * 2 / (1 << 20)} for k, v in sorted(out.items())}
    print(json.dumps(res, indent=1))
    return 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--fetch-size":
        return fetch_size(sys.argv[2])
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="residual_cost.json")
    ap.add_argument("--only", nargs="*", help='row ids ("C2 step 1", "C4 step 1", "C4 fused step 2")')
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed loop (even)")
    ap.add_argument("--warm-seconds", type=float, default=MIN_WARM_S, help="untimed loops of every kernel before the timed ones (0 under a counter run)")
    return measure(ap.parse_args())


if __name__ == "__main__":
    sys.exit(main())
