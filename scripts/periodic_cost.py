"""What --boundary periodic costs: the same sweep kernel with a fixed ring and with the periodic wrap in front of every launch, timed on one GPU
with HIP events, alternating fixed / periodic, several repeats each.

    python scripts/periodic_cost.py --out profiles/periodic_cost.json            # C4 headline, C2 tile, c4f64 4-stage pipeline
    python scripts/periodic_cost.py --boundary periodic reflect --out profiles/boundary_cost.json   # C4 headline and C2 tile, both modes in one run
    rocprofv3 --kernel-trace --stats -d TRACE -o c4 -- python scripts/periodic_cost.py --only c4 --repeats 2 --out /tmp/x.json
    python scripts/periodic_cost.py --summarize-trace TRACE --merge profiles/periodic_cost.json   # wrap kernel's own time (no GPU)

Every timed loop starts from the same finite input (the shipped coefficients sum to 1.5: a float array overflows after ~218 time steps, and
inf / NaN operands change the clocks), both variants share one arena laid out by Kernel.alloc_pair, and every timed kernel is verified once
(one launch against its gold kernel, and for periodic kernels the input's ring against the wrap of its interior).  The kernels are the ones
tests/periodic_cases.py lists (prebuilt by __graft_entry__.build()); nothing here runs hipcc."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MIN_WARM_S = 1.0


def torch_wrap(a, H):
    """The ring of `a` (a torch tensor) filled from its interior (tests/periodic_cases.host_wrap on the device)."""
    from periodic_cases import host_wrap
    return host_wrap(a, H)


def verify(torch, kern, A0, A, B, Ag, Bg):
    """One launch from A0 against the gold kernel (bit for bit, or within the tolerance for a reassociated pipeline); periodic: the input's
    ring against the wrap of A0's interior."""
    i = kern.info
    A.copy_(A0); B.zero_(); Ag.copy_(A0); Bg.zero_()
    kern.launch(A.data_ptr(), B.data_ptr())
    kern.launch_gold(Ag.data_ptr(), Bg.data_ptr())
    torch.cuda.synchronize()
    H = i["halo"]
    inner = tuple(slice(H, s - H) for s in B.shape)
    out = {}
    if i["arithmetic"] == "gold-order":
        out["dr_equals_gold"] = bool(torch.equal(B, Bg))
        ok = out["dr_equals_gold"]
    else:
        rel = ((B[inner].double() - Bg[inner].double()).abs() / Bg[inner].double().abs().clamp_min(1e-30)).max().item()
        out["dr_vs_gold_max_rel"] = rel
        ok = rel <= (1e-6 if i["dtype"] == "fp32" else 1e-12)
    if kern.periodic:
        Ag.copy_(A0)
        out["input_ring_is_wrap"] = bool(torch.equal(A, torch_wrap(Ag, H)))
        ok = ok and out["input_ring_is_wrap"]
    elif kern.fills_ring:
        from boundary_cases import host_fill
        a = host_fill(A0.cpu().numpy(), H, kern.boundaries)          # on the host: the mirror reads reversed slices
        out["input_ring_is_fill"] = bool(torch.equal(A.cpu(), torch.from_numpy(a)))
        del a
        ok = ok and out["input_ring_is_fill"]
    out["ok"] = bool(ok)
    return out


def measure(args):
    import torch
    import drstencil_amd as drs
    import bench
    from periodic_cases import cost_cases
    os.environ["DRS_NO_COMPILE"] = "1"
    dev = torch.device("cuda:0")
    rows = []
    modes = list(args.boundary)
    cases = cost_cases()
    if modes != ["periodic"]:       # the other modes are prebuilt for C4 headline and C2 tile (tests/boundary_cases.py)
        import boundary_cases
        cases = [c for c in cases if c[0] in [b[0] for b in boundary_cases.cost_cases()]]
    for cid, w, fixed_opts, per_opts in cases:
        if args.only and cid not in args.only:
            continue
        wl = bench.WORKLOADS[w]
        kf = drs.Kernel(fixed_opts + [wl["stc"]])
        kern = {"fixed": kf}
        for m in modes:
            kern[m] = drs.Kernel(fixed_opts + ["--boundary", m, wl["stc"]])
            assert kern[m].boundaries == (m,) * kf.info["ndim"] and not kf.fills_ring
        i = kf.info
        tdt = torch.float32 if i["dtype"] == "fp32" else torch.float64
        shape = (i["L"], i["M"], i["N"]) if i["ndim"] == 3 else (i["M"], i["N"])
        A, B, arena = kf.alloc_pair(torch, dev, dtype=tdt)          # one arena for both variants: the same placement
        g = torch.Generator(device=dev).manual_seed(1)
        A0 = torch.rand(shape, dtype=tdt, device=dev, generator=g)
        Ag, Bg = torch.empty_like(A0), torch.empty_like(A0)
        checks = {name: verify(torch, k, A0, A, B, Ag, Bg) for name, k in kern.items()}
        del Ag, Bg
        step = i["step"]
        launches = args.launches
        stream = torch.cuda.current_stream(dev)

        def loop(k):
            A.copy_(A0); B.zero_()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            n = k.run(A.data_ptr(), B.data_ptr(), iterations=launches * step, stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            assert n == launches
            return e0.elapsed_time(e1) / n
        names = ["fixed"] + modes
        for name in names:          # clocks up before anything is timed
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < MIN_WARM_S:
                loop(kern[name])
        ms = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                ms[name].append(loop(kern[name]))
        ups = kf.updates_per_launch()
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        row = {"id": cid, "workload": wl["name"], "options": " ".join(fixed_opts), "launches_per_loop": launches, "repeats": args.repeats,
               "ms_per_launch": {k: [round(x, 5) for x in v] for k, v in ms.items()},
               "median_ms_per_launch": {k: round(v, 5) for k, v in med.items()},
               "gstencil_per_s": {k: round(ups / (v * 1e-3) / 1e9, 2) for k, v in med.items()},
               "%s_over_fixed_gstencil" % modes[0]: round(med["fixed"] / med[modes[0]], 4),
               "wrap_ms_per_launch_by_difference": round(med[modes[0]] - med["fixed"], 5),
               "ring_elements": int(A0.numel() - ups // step),
               "verified": checks}
        for m in modes[1:]:
            row["%s_over_fixed_gstencil" % m] = round(med["fixed"] / med[m], 4)
        row["fixed_spread_ms"] = round(max(ms["fixed"]) - min(ms["fixed"]), 5)          # the fixed kernel's run-to-run spread in this run
        rows.append(row)
        print(json.dumps({k: row[k] for k in ["id", "median_ms_per_launch", "gstencil_per_s", "fixed_spread_ms", "verified"] + ["%s_over_fixed_gstencil" % m for m in modes]}), flush=True)
        del A, B, arena, A0
        torch.cuda.empty_cache()
    res = {"what": "fixed vs --boundary " + " / ".join(modes) + ", same sweep kernel, same arena, HIP events around run() of launches_per_loop launches, "
                   "alternating the variants, input restored before every loop; median over repeats",
           "device": torch.cuda.get_device_name(0), "target": "C4 periodic >= 0.93 of fixed GStencil/s", "cases": rows}
    c4 = [r for r in rows if r["id"] == "c4"]
    if c4 and modes[0] == "periodic":
        res["c4_target_met"] = c4[0]["periodic_over_fixed_gstencil"] >= 0.93
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    ok = all(r["verified"][k]["ok"] for r in rows for k in r["verified"])
    print("written %s, verified %s" % (args.out, ok))
    return 0 if ok else 1


def summarize_trace(args):
    """The wrap kernel's own time from a rocprofv3 --kernel-trace --stats run of `--only c4`, merged into --merge."""
    stats = sorted(glob.glob(os.path.join(args.summarize_trace, "**", "*kernel_stats.csv"), recursive=True))
    assert stats, "no *kernel_stats.csv under " + args.summarize_trace
    kernels = {}
    for row in csv.DictReader(open(stats[-1])):
        if row["Name"].startswith(("dr_", "wrap_", "gold_")):         # the generated kernels (torch's fills and copies are the harness)
            kernels[row["Name"]] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "total_ms": float(row["TotalDurationNs"]) / 1e6}
    res = json.load(open(args.merge))
    c4 = [r for r in res["cases"] if r["id"] == "c4"][0]
    wrap = {k: v for k, v in kernels.items() if k.startswith("wrap_")}
    sweep = {k: v for k, v in kernels.items() if k.startswith("dr_")}
    assert len(wrap) == 1 and len(sweep) == 1, kernels.keys()
    (wn, wv), (sn, sv) = list(wrap.items())[0], list(sweep.items())[0]
    esz = 4
    moved = 2 * esz * c4["ring_elements"]                  # every ring element read from the interior once and written once
    res["trace"] = {"source": os.path.basename(stats[-1]), "kernels": kernels, "wrap_kernel": wn, "wrap_average_us": round(wv["average_us"], 2),
                    "sweep_kernel": sn, "sweep_average_us": round(sv["average_us"], 2),
                    "wrap_over_sweep": round(wv["average_us"] / sv["average_us"], 4),
                    "wrap_bytes_moved": moved, "wrap_bytes_moved_what": "ring elements x 2 (read + write) x 4 bytes",
                    "wrap_GB_per_s": round(moved / (wv["average_us"] * 1e-6) / 1e9, 1)}
    # the sweep right after a wrap against the sweep right after a sweep (the fixed loop), from the per-dispatch trace
    traces = sorted(glob.glob(os.path.join(args.summarize_trace, "**", "*kernel_trace.csv"), recursive=True))
    if traces:
        rows = sorted(csv.DictReader(open(traces[-1])), key=lambda r: int(r["Start_Timestamp"]))
        after = {"wrap_": [], "dr_": []}
        for a, b in zip(rows, rows[1:]):
            if b["Kernel_Name"] == sn:
                for pre in after:
                    if a["Kernel_Name"].startswith(pre):
                        after[pre].append((int(b["End_Timestamp"]) - int(b["Start_Timestamp"])) / 1e3)
        med = {k: sorted(v)[len(v) // 2] for k, v in after.items() if v}
        if len(med) == 2:
            res["trace"].update({"sweep_after_wrap_median_us": round(med["wrap_"], 2), "sweep_after_sweep_median_us": round(med["dr_"], 2),
                                 "sweep_slowdown_after_wrap_us": round(med["wrap_"] - med["dr_"], 2)})
    with open(args.merge, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["trace"], indent=1))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="periodic_cost.json")
    ap.add_argument("--only", nargs="*", help="case ids (c4, c2, c4f64_temporal4)")
    ap.add_argument("--boundary", nargs="+", default=["periodic"], choices=["periodic", "reflect"],
                    help="the non-fixed modes to time against fixed (default: periodic; `periodic reflect` times both in one run, C4 and C2)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed loop (even; 20 x step 4 = 80 time steps stay finite in fp64, "
                                                              "20 x step 2 in fp32)")
    ap.add_argument("--summarize-trace", help="rocprofv3 output directory (no GPU needed)")
    ap.add_argument("--merge", help="with --summarize-trace: the periodic_cost.json to add the trace to")
    args = ap.parse_args()
    if args.summarize_trace:
        return summarize_trace(args)
    return measure(args)


if __name__ == "__main__":
    sys.exit(main())
