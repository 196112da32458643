"""Child process of tests/test_source_cpu.py: one emulated --source plugin (tests/emu) on THREE arrays placed flush against inaccessible
pages (footprint.Guarded), so an access outside any of them is a SIGSEGV.  TEST INFRASTRUCTURE.
usage: python source_child.py <job.json>.  Announces every phase on stdout, prints `FAIL <kind>: <what>` and exits 1 when a check fails.
The memory contract with a source term: a launch reads the cells of `in` its taps reach and the interior of `src` (with --time-order 2
the interior of `out` too), each such value reaching only its own cell, and writes the interior of `out`; the rings of `src` and `out`
are neither read nor written, and `src` is never written."""
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
from footprint_child import fail, phase  # noqa: E402
from source_cases import host_launch, load_emulated  # noqa: E402


def main(job):
    lib = load_emulated(job["so"])
    spec = oracle.Spec(job["stc"], job["ndim"], 1)
    dt = np.dtype(job["dtype"])
    order2 = bool(job.get("order2"))
    H = spec.halo
    inner = interior_slices(spec.shape, H)
    ring = ring_mask(spec.shape, H)
    P = poison(oracle.fill_random(spec.shape, dt), spec)           # NaN in every cell of `in` that no tap reads
    B0 = oracle.fill_random(spec.shape, dt, seed=12)               # finite values in out's interior (order 2 reads them) ...
    B0[ring] = nan_value(dt)                                       # ... and NaN in the whole of out's ring
    F0 = oracle.fill_random(spec.shape, dt, seed=13)               # finite source values in the interior, NaN in the whole of src's ring
    F0[ring] = nan_value(dt)
    ref = host_launch(spec, P.copy(), B0.copy(), F0, None, order2)
    assert not np.isnan(ref[inner]).any()
    for placement in job["placements"]:
        gA, gB, gF = (Guarded(spec.shape, dt, placement) for _ in range(3))
        A, B, F = gA.array, gB.array, gF.array
        for gold in (False, True):
            name = "%s-flush %s" % (placement, "gold" if gold else "dr")
            phase(name + " poison launch")
            A[...] = P
            B[...] = B0
            F[...] = F0
            fn = lib.drs_plugin_launch_gold_src if gold else lib.drs_plugin_launch_src
            if fn(A.ctypes.data, B.ctypes.data, F.ctypes.data, None) != 0:
                fail("mismatch", "the launch entry point returned an error")
            if np.isnan(B[inner]).any():
                fail("nan_leak", "%s: %d NaN in the output's interior (an unread cell of in, a ring cell of src or out, or a byte outside reached a store)"
                     % (name, int(np.isnan(B[inner]).sum())))
            if not is_poison(B)[ring].all():
                fail("ring_changed", "%s: %d cells of the output's ring were written" % (name, int((~is_poison(B))[ring].sum())))
            if not bit_equal(A, P):
                fail("input_changed", "%s: the input array was written" % name)
            if not bit_equal(F, F0):
                fail("source_changed", "%s: the source array was written" % name)
            if not np.array_equal(bits(B[inner]), bits(ref[inner])):
                fail("mismatch", "%s: the interior differs from the host reference" % name)
        for g in (gA, gB, gF):
            g.close()


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        job = json.load(f)
    phase("setup")
    main(job)
    print("DONE", flush=True)
