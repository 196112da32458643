"""Child process of tests/test_boundary_axes_cpu.py: one emulated plugin (tests/emu) with reflecting / per-axis boundaries on arrays
placed flush against inaccessible pages (footprint.Guarded) -- an access outside an array is a SIGSEGV, which is why this is a process
of its own.  TEST INFRASTRUCTURE on top of tests/footprint.py and tests/footprint_child.py.  usage: python boundary_child.py <job.json>.

The input holds NaN in every cell that is neither read by the sweep nor the source of a ring cell the sweep reads; the output is all
NaN.  One launch of dr and of gold, end-flush and start-flush: no NaN in the output's interior, the output's ring untouched, and the
input left exactly as host_fill leaves it -- which says that the ring cells of fixed axes outside the fill's destinations, like the
interior, are bit-unchanged."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
from boundary_cases import fill_destinations, host_fill  # noqa: E402
from footprint import Guarded, bit_equal, interior_slices, is_poison, nan_filled, nan_value, read_mask, ring_mask  # noqa: E402
from footprint_child import fail, load, phase  # noqa: E402


def poison_unneeded(A0, spec, modes):
    """A0 with NaN wherever the launch has no business reading: the cells the sweep reads of the FILLED array, traced back through
    the fill to the cells of the array as given."""
    H = spec.halo
    idx = np.arange(A0.size, dtype=np.int64).reshape(A0.shape)
    held = host_fill(idx.copy(), H, modes)                # which given cell each cell of the filled array holds
    needed = np.zeros(A0.size, bool)
    needed[held[read_mask(spec)]] = True
    P = np.ascontiguousarray(A0).copy()
    P.reshape(-1)[~needed] = nan_value(P.dtype)
    return P


def main(job):
    lib = load(job["so"])
    ndim, step, modes = job["ndim"], job["step"], tuple(job["modes"])
    spec = oracle.Spec(job["stc"], ndim, step)
    dt = np.dtype(job["dtype"])
    H = spec.halo
    A0 = (np.random.default_rng(5).random(spec.shape) * 2.0 - 1.0).astype(dt)
    P = poison_unneeded(A0, spec, modes)
    P_after = host_fill(P.copy(), H, modes)
    dest = fill_destinations(spec.shape, H, modes)
    assert bit_equal(P_after[~dest], P[~dest])
    B_ref = nan_filled(spec.shape, dt)
    oracle.sweep(spec, P_after, B_ref, contract=1)
    inner = interior_slices(spec.shape, H)
    assert not np.isnan(B_ref[inner]).any(), "the reference of the poison launch is not NaN-free"
    ring = ring_mask(spec.shape, H)
    for placement in job["placements"]:
        gA, gB = Guarded(spec.shape, dt, placement), Guarded(spec.shape, dt, placement)
        A, B = gA.array, gB.array
        for gold in (False, True):
            name = "%s-flush %s poison launch" % (placement, "gold" if gold else "dr")
            phase(name)
            A[...] = P
            B[...] = nan_filled(spec.shape, dt)
            fn = lib.drs_plugin_launch_gold if gold else lib.drs_plugin_launch
            if fn(A.ctypes.data, B.ctypes.data, None) != 0:
                fail("mismatch", "the launch entry point returned an error")
            if np.isnan(B[inner]).any():
                fail("nan_leak", "%s: %d NaN in the output's interior" % (name, int(np.isnan(B[inner]).sum())))
            if not is_poison(B)[ring].all():
                fail("ring_changed", "%s: the output's ring was written" % name)
            if not bit_equal(A[~dest], P[~dest]):
                fail("input_changed", "%s: a cell outside the fill's destinations (interior or the ring of a fixed axis) was written" % name)
            if not bit_equal(A, P_after):
                fail("mismatch", "%s: the input's ring is not the host fill" % name)
            if not np.array_equal(B[inner], B_ref[inner]):
                fail("mismatch", "%s: the interior differs from the oracle's sweep of the filled input" % name)
        gA.close()
        gB.close()


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        job = json.load(f)
    phase("setup")
    main(job)
    print("DONE", flush=True)
