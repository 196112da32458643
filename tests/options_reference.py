"""The host reference and the comparison of a run whose problem mode is read off the kernel's own options: reflecting and per-axis
boundaries, --source, --time-order 2 and their combinations (the fixed and periodic forms too).  Used by the shape x mode sample
(tests/test_shape_modes_cpu.py, tests/test_shape_modes_gpu.py), the special-value suite (tests/special_values.py) and the manual sweeps
(fuzz_parity.check_mode for --mode reflect | mixed | source | order2_source).  Nothing here computes a stencil: every reference is one
the suites already had -- source_cases.host_run, wave_cases.host_run, boundary_cases.oracle_boundary_run,
periodic_cases.oracle_periodic_run, oracle.sweep(..., contract=1)."""
import numpy as np

import oracle
from fuzz_parity import mode_inputs, rel_error, ring_mask, signed_random


def options_reference(spec, ndim, opts, A, B, F, launches):
    """The host reference of `launches` launches of the ping-pong loop of a kernel generated with `opts` (without the .stc), in place,
    by the existing reference of what the options name: source_cases.host_run (--source; F is the source array), wave_cases.host_run
    (--time-order 2, fixed or periodic), boundary_cases.oracle_boundary_run (reflecting and per-axis boundaries),
    periodic_cases.oracle_periodic_run, or the oracle's contracted sweep."""
    import boundary_cases, periodic_cases, source_cases, wave_cases
    modes = boundary_cases.modes_of(list(opts) + ["x"], ndim)
    order2 = "--time-order" in opts and opts[opts.index("--time-order") + 1] == "2"
    fixed, periodic = all(m == "fixed" for m in modes), all(m == "periodic" for m in modes)
    if "--source" in opts:
        return source_cases.host_run(spec, A, B, F, launches, modes, order2)
    if order2 and (fixed or periodic):
        return wave_cases.host_run(spec, A, B, launches, periodic=periodic)
    if not (fixed or periodic) or order2:
        return boundary_cases.oracle_boundary_run(spec, A, B, modes, launches, order2=order2)
    if periodic:
        return periodic_cases.oracle_periodic_run(spec, A, B, launches)
    for i in range(launches):
        src, dst = (A, B) if i % 2 == 0 else (B, A)
        oracle.sweep(spec, src, dst, contract=1)
    return launches


def compare_options_run(spec, ndim, opts, dtype, A0, B0, A, B, Ar, Br, launches, temporal):
    """(ok, rel) like fuzz_parity.compare_mode_run for a kernel with reflecting / per-axis boundaries or a source term
    (test_boundary_axes_gpu's rule): what neither a ring fill nor a sweep may write is bit-unchanged, the array filled last is its own
    host fill, and the arrays equal the reference's bit for bit -- within the dtype's bar for a temporal pipeline, which is not the gold
    kernel."""
    import boundary_cases
    modes = boundary_cases.modes_of(list(opts) + ["x"], ndim)
    h = spec.halo
    frozen = ring_mask(A0.shape, h) & ~boundary_cases.fill_destinations(A0.shape, h, modes)
    if not (np.array_equal(A[frozen], A0[frozen]) and np.array_equal(B[frozen], B0[frozen])):
        return False, 0.0
    filled = A if launches % 2 else B                        # the input of the last launch
    if any(m != "fixed" for m in modes) and not np.array_equal(filled, boundary_cases.host_fill(filled.copy(), h, modes)):
        return False, 0.0
    if not temporal:
        return bool(np.array_equal(A, Ar) and np.array_equal(B, Br)), 0.0
    rel = max(rel_error(A, Ar), rel_error(B, Br))
    return bool(rel <= (1e-6 if dtype == "fp32" else 1e-12)), rel


def check_options(job, k, torch):
    """One job (ndim, stc, dtype, arguments, step) on the GPU, whatever its mode: Kernel.run for the spec's iterations from random A, B
    (and F) against options_reference, then the gold kernel from the same inputs against the same reference (always bit for bit).
    ("ok" | "bad", temporal, max relative error), as fuzz_parity.check returns."""
    ndim, stc, dtype, args, step = job
    opts = args[:-1]
    temporal = k.info.get("stages", 1) > 1
    source = "--source" in opts
    assert k.source == source and not (temporal and (source or k.time_order == 2)), "an order-2 or source kernel with on-chip stages"
    import boundary_cases
    assert k.boundaries == boundary_cases.modes_of(args, ndim) and k.time_order == (2 if "--time-order" in opts else 1)
    spec = oracle.Spec(stc, ndim, step)
    A0, B0 = mode_inputs(spec, dtype, temporal)
    F0 = signed_random(spec.shape, A0.dtype, 13) if source else None
    Ar, Br = A0.copy(), B0.copy()
    launches = options_reference(spec, ndim, opts, Ar, Br, F0, spec.launches)
    status, worst = "ok", 0.0
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        dF = torch.from_numpy(F0).cuda() if source else None
        n = k.run(dA.data_ptr(), dB.data_ptr(), gold=gold, **({"d_src": dF.data_ptr()} if source else {}))
        torch.cuda.synchronize()
        ok, rel = compare_options_run(spec, ndim, opts, dtype, A0, B0, dA.cpu().numpy(), dB.cpu().numpy(), Ar, Br, launches, temporal and not gold)
        worst = max(worst, rel)
        if n != launches or not ok or (source and not np.array_equal(dF.cpu().numpy(), F0)):
            status = "bad"
    return status, temporal, worst
