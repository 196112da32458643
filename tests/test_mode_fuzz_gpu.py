"""--boundary periodic and --time-order 2 over the tuner's space on the MI355X: the fixed random sample of tests/mode_fuzz_cases.py
(about 20 configurations per mode, both dtypes, prefetch depths 1-4, periodic steps 1-3) through the mode-aware check of
tests/fuzz_parity.py -- Kernel.run and the gold kernel from random A and random B against the oracle with the host wrap in front of
every launch and / or the subtraction of the old output behind it, bit for bit for single-pass kernels, within 1e-6 (fp32) / 1e-12
(fp64) for on-chip temporal pipelines -- and the edge grids: the smallest legal periodic grids, a grid narrower than a tile, a
wavefront's row and a vector in every direction, an interior of whole tiles plus one column.  What the emulation cannot see is
checked here: the gfx950 compiler's handling of the old-value loads, their register sets and guards.  Every kernel is prebuilt by
__graft_entry__.build(): nothing here starts hipcc."""
import time

import numpy as np
import pytest

import oracle
from mode_fuzz_cases import EDGE, MIN_CHECKED, MODES, ROLL_IDS, sample_jobs
from periodic_cases import roll_reference

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


@pytest.mark.parametrize("mode", MODES)
def test_mode_sampled_fuzz(torch_cuda, mode):
    """Kernels the runtime refuses (scratch or SGPR spills, an LDS limit, an invalid tile: decided when build() compiled them) count as
    refused, every other one must come out "ok"; at least three quarters of the sample is checked."""
    import drstencil_amd as drs
    import fuzz_parity
    jobs = sample_jobs(mode)
    checked = refused = 0
    t0 = time.time()
    for job in jobs:
        assert fuzz_parity.job_mode(job[3]) == mode
        try:
            k = drs.Kernel(job[3])           # cache hit: built by build(), before HIP was initialised
        except drs.KernelBuildError as e:
            assert "scratch" in str(e) or "Invalid configuration" in str(e) or "tile" in str(e), str(e)[-300:]
            refused += 1
            continue
        status, temporal, rel = fuzz_parity.check(job, k, torch_cuda)
        assert status == "ok", "%s (%s, temporal=%s, rel=%g)" % (" ".join(job[3]), status, temporal, rel)
        checked += 1
    print("mode fuzz %s: %d checked, %d refused, %.1f s" % (mode, checked, refused, time.time() - t0))
    assert checked >= MIN_CHECKED and checked + refused == len(jobs)


@pytest.mark.parametrize("cid,ndim,stc,opts,mode", EDGE, ids=[c[0] for c in EDGE])
def test_mode_edge_grids(torch_cuda, cid, ndim, stc, opts, mode):
    """Kernel.run for the spec's iterations, dr and gold, from random A and random B in [-1, 1): both arrays bit for bit against the
    host reference of the mode (rings included: unchanged under a fixed boundary, the host wrap under a periodic one)."""
    import drstencil_amd as drs
    import fuzz_parity
    torch = torch_cuda
    kern = drs.Kernel(opts + [stc])
    step = int(opts[opts.index("--step") + 1]) if "--step" in opts else 1
    dtype = "fp32" if "fp32" in opts else "fp64"
    spec = oracle.Spec(stc, ndim, step)
    H = spec.halo
    assert kern.info["stages"] == 1 and kern.info["halo"] == H
    assert kern.periodic == mode.endswith("periodic") and kern.time_order == (2 if mode.startswith("order2") else 1)
    if kern.periodic:
        assert kern.info["period"] == [d - 2 * H for d in spec.shape]
    A0, B0 = fuzz_parity.mode_inputs(spec, dtype, False)
    Ar, Br = A0.copy(), B0.copy()
    launches = fuzz_parity.mode_reference(spec, Ar, Br, spec.launches, mode)
    inner = tuple(slice(H, s - H) for s in spec.shape)
    assert not np.array_equal(Br[inner], B0[inner]) and not np.array_equal(Ar[inner], A0[inner])
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        assert kern.run(dA.data_ptr(), dB.data_ptr(), gold=gold) == launches
        torch.cuda.synchronize()
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        ok, _ = fuzz_parity.compare_mode_run(spec, mode, dtype, A0, B0, A, B, Ar, Br, launches, False)
        assert ok, (cid, gold, int((A != Ar).sum()), int((B != Br).sum()))
        if cid in ROLL_IDS and not gold:
            # oracle-free: launches x step periodic one-step updates by np.roll over the period, fp64
            ref = roll_reference(oracle.Spec(stc, ndim, 1).points, A0[inner], launches * step)
            assert fuzz_parity.rel_error(A[inner], ref) <= 1e-12, cid
