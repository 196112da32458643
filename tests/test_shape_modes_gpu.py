"""Random stencil shapes in every problem mode on the MI355X: the 12 committed shapes of tests/shape_mode_cases.py (one-sided along the
streamed dimension, without a centre, mixed signs; 2D and 3D, orders 1 and 2), each with one random configuration
of the tuner's space per mode -- fixed, periodic, reflect, a per-axis triple, order 2, source, order 2 + source, and the last with a
per-axis triple -- through Kernel.run for the spec's iterations and the gold kernel, against the host references of
tests/fuzz_parity.py and tests/options_reference.py: bit for bit for single-pass kernels, within 1e-6 (fp32) / 1e-12 (fp64) for on-chip temporal pipelines.  The
emulated suite (tests/test_shape_modes_cpu.py) checks the emitter's text on these shapes; what hipcc and the GPU make of the old-value
and source streams of a shape whose taps all lie ahead of the output plane is checked here.  Every kernel is prebuilt by
__graft_entry__.build(): nothing here starts hipcc."""
import time

import pytest

import shape_mode_cases as sm

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


@pytest.mark.parametrize("mode", sm.MODES)
def test_shape_modes(torch_cuda, mode):
    """Kernels that the generator or the runtime refused when build() compiled them (a --dist without data to reuse, an LDS demand
    beyond the limit, a spill, an unreadable resource report) count as refused, never as checked, and only with one of those messages;
    every other one must come out "ok";
    at least three quarters of the mode's sample is checked."""
    import drstencil_amd as drs
    import fuzz_parity
    jobs = sm.sample_jobs(mode)
    assert len(jobs) == sm.N_SHAPES
    checked, refused = 0, []
    t0 = time.time()
    for sid, ndim, stc, dims, dtype, opts, step in jobs:
        try:
            k = drs.Kernel(opts + [stc])           # cache hit: built by build(), before HIP was initialised
        except drs.KernelBuildError as e:
            assert "not in the cache" not in str(e), str(e)[-300:]       # every kernel of the sample was built, or refused, by build()
            assert any(k in str(e) for k in sm.KNOWN_REFUSALS + sm.RUNTIME_REFUSALS), str(e)[-300:]
            refused.append(sid)
            continue
        assert (k.info.get("stages", 1) == 1) or mode in ("fixed", "periodic", "reflect", "mixed"), sid
        job = (ndim, stc, dtype, opts + [stc], step)
        status, temporal, rel = fuzz_parity.check(job, k, torch_cuda)
        print("%s: %s%s" % (sid, status, ", temporal rel %.3g" % rel if temporal else ""))
        assert status == "ok", "%s: %s (%s, temporal=%s, rel=%g)" % (sid, " ".join(opts), status, temporal, rel)
        checked += 1
    print("shape fuzz %s: %d checked, %d refused %s, %.1f s" % (mode, checked, len(refused), refused, time.time() - t0))
    assert checked >= sm.MIN_CHECKED and checked + len(refused) == len(jobs), (mode, checked, refused)
