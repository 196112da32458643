"""Child process of tests/test_time_order_cpu.py: one emulated --time-order 2 plugin (tests/emu) on arrays placed flush against
inaccessible pages (footprint.Guarded), so an access outside either array is a SIGSEGV.  TEST INFRASTRUCTURE.
usage: python wave_child.py <job.json>.  Announces every phase on stdout, prints `FAIL <kind>: <what>` and exits 1 when a check fails.
The extended memory contract: a launch reads the cells of `in` its taps reach and the interior of `out`, each old value reaching only
its own cell, and writes the interior of `out`; out's ring is neither read nor written."""
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
from footprint import Guarded, bit_equal, bits, interior_slices, is_poison, nan_value, poison, ring_mask  # noqa: E402
from footprint_child import fail, load, phase  # noqa: E402
from wave_cases import host_launch  # noqa: E402


def main(job):
    lib = load(job["so"])
    spec = oracle.Spec(job["stc"], job["ndim"], 1)
    dt = np.dtype(job["dtype"])
    H = spec.halo
    inner = interior_slices(spec.shape, H)
    ring = ring_mask(spec.shape, H)
    P = poison(oracle.fill_random(spec.shape, dt), spec)           # NaN in every cell of `in` that no tap reads
    B0 = oracle.fill_random(spec.shape, dt, seed=12)               # finite old values in out's interior ...
    B0[ring] = nan_value(dt)                                       # ... and NaN in the whole of out's ring
    ref = host_launch(spec, P.copy(), B0.copy())
    assert not np.isnan(ref[inner]).any()
    for placement in job["placements"]:
        gA, gB = Guarded(spec.shape, dt, placement), Guarded(spec.shape, dt, placement)
        A, B = gA.array, gB.array
        for gold in (False, True):
            name = "%s-flush %s" % (placement, "gold" if gold else "dr")
            phase(name + " poison launch")
            A[...] = P
            B[...] = B0
            fn = lib.drs_plugin_launch_gold if gold else lib.drs_plugin_launch
            if fn(A.ctypes.data, B.ctypes.data, None) != 0:
                fail("mismatch", "the launch entry point returned an error")
            if np.isnan(B[inner]).any():
                fail("nan_leak", "%s: %d NaN in the output's interior (an unread cell of in, out's ring or a byte outside reached a store)"
                     % (name, int(np.isnan(B[inner]).sum())))
            if not is_poison(B)[ring].all():
                fail("ring_changed", "%s: %d cells of the output's ring were written" % (name, int((~is_poison(B))[ring].sum())))
            if not bit_equal(A, P):
                fail("input_changed", "%s: the input array was written" % name)
            if not np.array_equal(bits(B[inner]), bits(ref[inner])):
                fail("mismatch", "%s: the interior differs from S(in) - out_old" % name)
        gA.close()
        gB.close()


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        job = json.load(f)
    phase("setup")
    main(job)
    print("DONE", flush=True)
