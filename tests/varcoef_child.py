"""Child process of tests/test_varcoef_cpu.py: one emulated --varcoef plugin (tests/emu) with `in`, `out`, `src`, `coef` and (with
--residual max) a residual array of exactly residual_elems elements, each placed flush against inaccessible pages (footprint.Guarded), so
an access outside any of them is a SIGSEGV.  TEST INFRASTRUCTURE.  No sanitizer and nothing preloaded: the pages are the check.
usage: python varcoef_child.py <job.json>.  Announces every phase on stdout, prints `FAIL <kind>: <what>` and exits 1 when a check fails.
The memory contract with the option: a launch additionally reads the INTERIOR of each of the T coefficient grids, each value reaching its
own cell and tap only; the ring of every grid is NaN here (a ring value that reached a stored cell would show in the arrays) and coef is
never written."""
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
import residual_cases as rc  # noqa: E402
import varcoef_cases as vc  # noqa: E402
from footprint import Guarded, bit_equal, nan_value, ring_mask  # noqa: E402
from footprint_child import fail, phase  # noqa: E402


def main(job):
    lib = vc.load_emulated(job["so"])
    opts, ndim = job["opts"], job["ndim"]
    spec = oracle.Spec(job["stc"], ndim, 1)
    dt = np.dtype(vc.dtype_of(opts))
    fills = "--boundary" in " ".join(opts)
    ring = ring_mask(spec.shape, spec.halo)
    A0, B0, F0, _, _, K0 = vc.inputs(spec, opts)
    if not fills:                      # with a ring fill the launch itself rewrites in's ring; otherwise NaN where nothing may be read
        A0 = rc.poisoned_input(A0, spec)
    B0[ring] = nan_value(dt)
    if F0 is not None:
        F0[ring] = nan_value(dt)
    K0[:, ring] = nan_value(dt)
    Ar, Br = A0.copy(), B0.copy()
    want = vc.host_launch(spec, ndim, opts, Ar, Br, F0, None, None, K0)
    if np.isnan(vc.interior(Br, spec.halo)).any() or not np.isfinite(want):
        fail("reference", "the host reference is not finite")
    for placement in job["placements"]:
        gA, gB = (Guarded(spec.shape, dt, placement) for _ in range(2))
        gK = Guarded(K0.shape, dt, placement)
        gF = Guarded(spec.shape, dt, placement) if F0 is not None else None
        gR = Guarded((lib.residual_elems,), dt, placement) if lib.residual_elems else None
        A, B, K = gA.array, gB.array, gK.array
        F = gF.array if gF else None
        R = gR.array if gR else None
        phase("%s-flush launch" % placement)
        A[...] = A0
        B[...] = B0
        K[...] = K0
        if R is not None:
            R[...] = np.nan
        if F is not None:
            F[...] = F0
        if lib.launch(A, B, F, R, None, None, K) != 0:
            fail("mismatch", "the launch entry point returned an error")
        if not bit_equal(A, Ar) or not bit_equal(B, Br):
            fail("mismatch", "%s: the arrays differ from the host reference (out's ring included)" % placement)
        if not bit_equal(K, K0):
            fail("coef_changed", "%s: the coefficient array was written" % placement)
        if F is not None and not bit_equal(F, F0):
            fail("source_changed", "%s: the source array was written" % placement)
        if R is not None:
            if not rc.same_bits(R[0], want):
                fail("residual", "%s: r = %r, the reference has %r" % (placement, R[0], want))
            if np.isnan(R).any():
                fail("partials", "%s: %d elements of d_res were not written" % (placement, int(np.isnan(R).sum())))
        for g in (gA, gB, gF, gR, gK):
            if g:
                g.close()


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        job = json.load(f)
    phase("setup")
    main(job)
    print("DONE", flush=True)
