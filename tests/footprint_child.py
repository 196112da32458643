"""Child process of tests/test_memory_footprint_cpu.py: runs one emulated plugin (tests/emu) on arrays placed flush against
inaccessible pages (footprint.Guarded) -- an access outside an array is a SIGSEGV, which is why this is a process of its own.
TEST INFRASTRUCTURE.  usage: python footprint_child.py <job.json>.  Announces every phase on stdout before entering it (the parent
reports the last one when the process dies), prints `FAIL <kind>: <what>` and exits 1 when a check fails, exits 0 otherwise.
Kinds: mismatch (values differ from the oracle), nan_leak (an unread cell reached a stored output), ring_changed (the output's ring
was written), input_changed (the input was written)."""
import ctypes
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
from footprint import Guarded, bit_equal, bits, interior_slices, is_poison, nan_filled, poison, poison_periodic, ring_mask  # noqa: E402
from periodic_cases import host_wrap, oracle_periodic_run  # noqa: E402


def phase(text):
    print("PHASE " + text, flush=True)


def fail(kind, text):
    print("FAIL %s: %s" % (kind, text), flush=True)
    sys.exit(1)


def load(so):
    lib = ctypes.CDLL(so)
    for n in ("drs_plugin_launch", "drs_plugin_launch_gold"):
        getattr(lib, n).argtypes = [ctypes.c_void_p] * 3
    lib.drs_plugin_info.restype = ctypes.c_char_p
    return lib


def ping_pong(fn, A, B, iterations, step):
    n = t = 0
    while t < iterations:
        if fn(A.ctypes.data, B.ctypes.data, None) != 0 or fn(B.ctypes.data, A.ctypes.data, None) != 0:
            fail("mismatch", "the launch entry point returned an error")
        n += 2
        t += 2 * step
    return n


def compare(what, spec, got, ref, bar, ring_exact=True):
    """bar None: bit for bit.  Otherwise: the interior within `bar` (relative, the project's checkError metric), the ring bit for bit
    (ring_exact=False: a periodic pipeline's second array, whose ring the wrap filled from an interior that is itself within `bar`)."""
    if bar is None:
        if not bit_equal(got, ref):
            diff = bits(got) != bits(ref)
            in_ring = diff & ring_mask(got.shape, spec.halo)
            if in_ring.any():
                fail("ring_changed", "%s: %d cells of the ring differ from the oracle's, first at %s" % (what, int(in_ring.sum()), tuple(np.argwhere(in_ring)[0])))
            fail("mismatch", "%s differs from the oracle in %d cells, first at %s" % (what, int(diff.sum()), tuple(np.argwhere(diff)[0])))
        return
    rel = oracle.check(spec, got, ref)["max_rel"]
    print("INFO %s max_rel %.3g (bar %g)" % (what, rel, bar), flush=True)
    if not rel < bar:
        fail("mismatch", "%s: max_rel %.3g beyond %g" % (what, rel, bar))
    ring = ring_mask(got.shape, spec.halo)
    if ring_exact and not np.array_equal(bits(got)[ring], bits(ref)[ring]):
        fail("ring_changed", "%s: the ring differs from the oracle's" % what)


def check_poison_launch(what, spec, A, B, A_expect, B_ref, bar):
    h = spec.halo
    inner = interior_slices(B.shape, h)
    ring = ring_mask(B.shape, h)
    if np.isnan(B[inner]).any():
        fail("nan_leak", "%s: %d NaN in the output's interior, first at %s (an unread cell or a byte outside the arrays reached a store)"
             % (what, int(np.isnan(B[inner]).sum()), tuple(np.argwhere(np.isnan(B[inner]))[0] + h)))
    if not is_poison(B)[ring].all():
        fail("ring_changed", "%s: %d cells of the output's ring were written, first at %s"
             % (what, int((~is_poison(B))[ring].sum()), tuple(np.argwhere(~is_poison(B) & ring)[0])))
    if not bit_equal(A, A_expect):
        fail("input_changed", "%s: the input array differs in %d cells from what the launch may leave there" % (what, int((bits(A) != bits(A_expect)).sum())))
    if bar is None:
        if not np.array_equal(bits(B[inner]), bits(B_ref[inner])):
            fail("mismatch", "%s: the interior differs from the oracle's sweep of the poisoned input" % what)
    else:
        rel = oracle.check(spec, B, B_ref)["max_rel"]
        print("INFO %s max_rel %.3g (bar %g)" % (what, rel, bar), flush=True)
        if not rel < bar:
            fail("mismatch", "%s: max_rel %.3g beyond %g" % (what, rel, bar))


def sweep_job(job):
    lib = load(job["so"])
    info = json.loads(lib.drs_plugin_info().decode())
    ndim, step = job["ndim"], job["step"]
    spec = oracle.Spec(job["stc"], ndim, step)
    dt = np.dtype(job["dtype"])
    periodic = bool(job.get("periodic"))
    pipeline = bool(job.get("temporal")) and info.get("stages", 1) > 1
    dr_bar = (1e-6 if dt == np.float32 else 1e-12) if pipeline else None
    H = spec.halo
    A0 = oracle.fill_random(spec.shape, dt)
    B0 = oracle.fill_random(spec.shape, dt, seed=12) if periodic else np.zeros_like(A0)
    A_ref, B_ref = A0.copy(), B0.copy()
    n_ref = oracle_periodic_run(spec, A_ref, B_ref) if periodic else oracle.run(spec, A_ref, B_ref, contract=1)
    if periodic:
        P = poison_periodic(A0, spec)
        P_after = host_wrap(P.copy(), H)
    else:
        P = poison(A0, spec)
        P_after = P
    Bp_ref = nan_filled(spec.shape, dt)
    oracle.sweep(spec, P_after, Bp_ref, contract=1)
    assert not np.isnan(spec.interior(Bp_ref)).any(), "the reference of the poison launch is not NaN-free"
    for placement in job["placements"]:
        gA, gB = Guarded(spec.shape, dt, placement), Guarded(spec.shape, dt, placement)
        A, B = gA.array, gB.array
        for gold in (False, True):
            name = "%s-flush %s" % (placement, "gold" if gold else "dr")
            fn = lib.drs_plugin_launch_gold if gold else lib.drs_plugin_launch
            bar = None if gold else dr_bar
            phase(name + " ping-pong run")
            A[...] = A0
            B[...] = B0
            n = ping_pong(fn, A, B, spec.iterations, step)
            if n != n_ref or n != spec.launches:
                fail("mismatch", "%d launches, the oracle ran %d" % (n, n_ref))
            compare(name + " run A", spec, A, A_ref, bar)
            compare(name + " run B", spec, B, B_ref, bar, ring_exact=not periodic)
            if periodic and bar is not None and not bit_equal(B, host_wrap(B.copy(), H)):
                fail("ring_changed", name + " run B: the ring is not the image of the interior")
            phase(name + " poison launch")
            A[...] = P
            B[...] = nan_filled(spec.shape, dt)
            if fn(A.ctypes.data, B.ctypes.data, None) != 0:
                fail("mismatch", "the launch entry point returned an error")
            check_poison_launch(name + " poison launch", spec, A, B, P_after, Bp_ref, bar)
        gA.close()
        gB.close()


def wrap_job(job):
    lib = load(job["so"])
    lib.drs_plugin_wrap.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    info = json.loads(lib.drs_plugin_info().decode())
    H = info["halo"]
    dt = np.dtype(job["dtype"])
    shape = tuple(job["shape"])
    a0 = np.random.default_rng(7).random(shape).astype(dt)
    ref = np.pad(a0[interior_slices(shape, H)], H, mode="wrap")
    for placement in job["placements"]:
        g = Guarded(shape, dt, placement)
        for ring in ("seeded", "NaN"):
            phase("%s-flush wrap, %s ring" % (placement, ring))
            g.array[...] = a0
            if ring == "NaN":
                g.array[ring_mask(shape, H)] = nan_filled((1,), dt)[0]
            if lib.drs_plugin_wrap(g.array.ctypes.data, None) != 0:
                fail("mismatch", "drs_plugin_wrap returned an error")
            if np.isnan(g.array).any():
                fail("nan_leak", "the wrap left or copied NaN")
            if not bit_equal(g.array, ref):
                fail("mismatch", "the wrapped array differs from np.pad(interior, Halo, 'wrap')")
        g.close()


def pair_job(job):
    lib = load(job["so"])
    lib.drs_plugin_launch_pair.argtypes = [ctypes.c_void_p] * 5
    spec = oracle.Spec(job["stc"], job["ndim"], job["step"])
    dt = np.dtype(job["dtype"])
    a0 = oracle.fill_random(spec.shape, dt)
    a1 = (a0[::-1] * dt.type(0.5)).copy()
    inner = interior_slices(spec.shape, spec.halo)
    for placement in job["placements"]:
        g = [Guarded(spec.shape, dt, placement) for _ in range(4)]
        i0, o0, i1, o1 = (x.array for x in g)
        for poisoned in (False, True):
            name = "%s-flush pair launch%s" % (placement, ", poisoned" if poisoned else "")
            phase(name)
            ins = [poison(a, spec) if poisoned else a for a in (a0, a1)]
            fill = nan_filled(spec.shape, dt) if poisoned else oracle.fill_random(spec.shape, dt, seed=5)
            i0[...], i1[...] = ins
            o0[...] = fill
            o1[...] = fill
            if lib.drs_plugin_launch_pair(i0.ctypes.data, o0.ctypes.data, i1.ctypes.data, o1.ctypes.data, None) != 0:
                fail("mismatch", "drs_plugin_launch_pair returned an error")
            for k, (src, got_in, out) in enumerate(((ins[0], i0, o0), (ins[1], i1, o1))):
                ref = fill.copy()
                oracle.sweep(spec, src, ref, contract=1)
                if poisoned:
                    check_poison_launch("%s, pair %d" % (name, k), spec, got_in, out, src, ref, None)
                else:
                    if not bit_equal(got_in, src):
                        fail("input_changed", "%s, pair %d" % (name, k))
                    compare("%s, pair %d" % (name, k), spec, out, ref, None)
            if np.array_equal(o0[inner], o1[inner]):
                fail("mismatch", name + ": both pairs hold the same output")
        for x in g:
            x.close()


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        job = json.load(f)
    phase("setup")
    {"sweep": sweep_job, "wrap": wrap_job, "pair": pair_job}[job["mode"]](job)
    print("DONE", flush=True)
