"""IEEE special values inside the footprint, on the MI355X: the single-pass kernels that __graft_entry__.build() prebuilds for the other
GPU suites (special_values.gpu_cases: the non-temporal cases of gpu_cases.SMALL, periodic_cases.SMALL, boundary_cases.gpu_small_cases(),
wave_cases.SMALL, source_cases.SMALL + BOTH and the thin / tile_plus1 / min edge grids) on data that holds +-0.0, subnormals, values up
to the largest finite one, +-inf and NaN (special_values.special_fill; the source array too), two launches of dr_ and of gold_ (both
directions of the ping-pong) against the existing host references.  The comparison is special_values.same_bits on both whole arrays:
NaN in the same cells, every other cell the same bits, so the sign of a zero and every subnormal count -- what the packed FMAs, the
DPP shifts that insert 0 at the ends of a row and the buffer loads that return 0 outside the window make of such data is seen here
and nowhere else.  Kernels with on-chip stages (info["stages"] > 1) are left out: they are held to a relative bar, which means nothing
on this data.  Nothing here starts hipcc."""
import numpy as np
import pytest

import oracle
import special_values as sv

pytestmark = pytest.mark.gpu
CASES = sv.gpu_cases()


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


@pytest.mark.parametrize("cid,ndim,stc,opts", CASES, ids=[c[0] for c in CASES])
def test_special_values_bit_for_bit(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    torch = torch_cuda
    kern = drs.Kernel(opts + [stc])
    assert kern.info["stages"] == 1, cid
    spec = oracle.Spec(stc, ndim, sv.step_of(opts))
    A0, B0, F0 = sv.inputs(cid, spec, opts)
    Ar, Br = sv.reference(spec, ndim, opts, A0.copy(), B0.copy(), F0)
    share = sv.assert_conditions(cid, spec, Ar, Br)
    dF = torch.from_numpy(F0).cuda() if F0 is not None else None
    src = {"d_src": dF.data_ptr()} if F0 is not None else {}
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        fn = kern.launch_gold if gold else kern.launch
        fn(dA.data_ptr(), dB.data_ptr(), **src)
        fn(dB.data_ptr(), dA.data_ptr(), **src)
        torch.cuda.synchronize()
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        print("%s %s: finite share %.3f, cells that differ: A %d, B %d" % (cid, "gold" if gold else "dr", share, sv.count_different(A, Ar), sv.count_different(B, Br)))
        assert sv.same_bits(A, Ar) and sv.same_bits(B, Br), (cid, gold, sv.count_different(A, Ar), sv.count_different(B, Br))
        if F0 is not None:
            assert sv.same_bits(dF.cpu().numpy(), F0), (cid, gold)
