"""--boundary periodic on the MI355X: the wrap kernel and periodic sweeps against the CPU oracle with the ring filled from the interior
before every launch (bit for bit for single-pass kernels, within 1e-6 fp32 / 1e-12 fp64 for on-chip temporal pipelines), the gold entry
point, full-size C4 / C2 (byte offsets past 2^32), and an oracle-free np.roll reference.  Every kernel is prebuilt by
__graft_entry__.build() (tests/periodic_cases.py): nothing here starts hipcc."""
import numpy as np
import pytest

import oracle
from periodic_cases import ROLL, SMALL, full_cases, host_wrap, oracle_periodic_run, roll_reference

pytestmark = pytest.mark.gpu
REL_TOL = {"fp32": 1e-6, "fp64": 1e-12}


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


def _dtype(opts):
    return "fp32" if "fp32" in opts else "fp64"


def _step(opts):
    return int(opts[opts.index("--step") + 1]) if "--step" in opts else 1


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)))


@pytest.mark.parametrize("cid,ndim,stc,opts", SMALL, ids=[c[0] for c in SMALL])
def test_periodic_small_vs_oracle_with_wrap(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    torch = torch_cuda
    dt = _dtype(opts)
    npdt = np.float32 if dt == "fp32" else np.float64
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, _step(opts))
    H = spec.halo
    assert kern.periodic and kern.info["halo"] == H
    assert kern.info["period"] == [d - 2 * H for d in spec.shape]
    temporal = kern.info["stages"] > 1
    A0 = oracle.fill_random(spec.shape, npdt)
    B0 = oracle.fill_random(spec.shape, npdt, seed=9)         # the output's ring: values no launch may read or write
    # one launch: in's ring becomes the wrap of in's interior, in's interior stays, out's ring stays, out's interior = oracle
    dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
    kern.launch(dA.data_ptr(), dB.data_ptr())
    torch.cuda.synchronize()
    A1, B1 = dA.cpu().numpy(), dB.cpu().numpy()
    Aw = host_wrap(A0.copy(), H)
    assert np.array_equal(A1, Aw), cid
    Bref = B0.copy()
    oracle.sweep(spec, Aw, Bref, contract=1)
    ring = np.ones(A0.shape, bool)
    ring[tuple(slice(H, s - H) for s in A0.shape)] = False
    assert np.array_equal(B1[ring], B0[ring]), cid
    if temporal:
        assert _rel(B1, Bref) <= REL_TOL[dt], cid
    else:
        assert np.array_equal(B1, Bref), cid
    # the spec's whole ping-pong run (Kernel.run) and the gold entry point, against the oracle run with the wrap before every launch
    Ar, Br = A0.copy(), B0.copy()
    n_ref = oracle_periodic_run(spec, Ar, Br)
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        n = kern.run(dA.data_ptr(), dB.data_ptr(), gold=gold)
        torch.cuda.synchronize()
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        assert n == n_ref
        if temporal and not gold:
            assert _rel(A, Ar) <= REL_TOL[dt] and _rel(B, Br) <= REL_TOL[dt], cid
            assert np.array_equal(A[ring], Ar[ring])              # filled from A0's interior: exact
        else:
            assert np.array_equal(A, Ar) and np.array_equal(B, Br), (cid, gold)


def test_wrap_full_c4_past_4gib(torch_cuda):
    """Kernel.wrap on a whole C4 fp32 array (4 GiB: the top ghost planes lie beyond 2^32 bytes) == the host wrap, bit for bit."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = full_cases()[0]
    kern = drs.Kernel(opts + [stc])
    i = kern.info
    H = i["halo"]
    g = torch.Generator(device="cuda").manual_seed(4321)
    A = torch.rand((i["L"], i["M"], i["N"]), dtype=torch.float32, device="cuda", generator=g)
    a = A.cpu().numpy()
    kern.wrap(A.data_ptr())
    torch.cuda.synchronize()
    host_wrap(a, H)
    assert np.array_equal(A.cpu().numpy(), a)


@pytest.mark.parametrize("case", [0, 1], ids=["C4_headline", "C2_tile"])
def test_full_size_periodic_launch(torch_cuda, case):
    """BASELINE sizes, periodic, one launch on a seeded input: the whole grid against the oracle-with-wrap bit for bit, dr == gold."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = full_cases()[case]
    kern = drs.Kernel(opts + [stc])
    i = kern.info
    H = i["halo"]
    assert kern.periodic and i["arithmetic"] == "gold-order"
    shape = (i["L"], i["M"], i["N"]) if ndim == 3 else (i["M"], i["N"])
    g = torch.Generator(device="cuda").manual_seed(1234)
    A0 = torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)
    A, B = A0.clone(), torch.zeros_like(A0)
    Ag, Bg = A0.clone(), torch.zeros_like(A0)
    kern.launch(A.data_ptr(), B.data_ptr())
    kern.launch_gold(Ag.data_ptr(), Bg.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(A, Ag) and torch.equal(B, Bg), cid
    del Ag, Bg
    a = host_wrap(A0.cpu().numpy(), H)
    del A0
    assert np.array_equal(A.cpu().numpy(), a), cid
    del A
    b = np.zeros_like(a)
    spec = oracle.Spec(stc, ndim, _step(opts))
    oracle.sweep(spec, a, b, contract=1)
    del a
    assert np.array_equal(B.cpu().numpy(), b), cid


def test_run_equals_roll_reference(torch_cuda):
    """Kernel.run for the spec's iterations (fused step 2, fp64) == that many periodic one-step updates by np.roll, within 1e-12."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = ROLL
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, _step(opts))
    H = spec.halo
    A0 = oracle.fill_random(spec.shape, np.float64)
    dA, dB = torch.from_numpy(A0).cuda(), torch.zeros(spec.shape, dtype=torch.float64, device="cuda")
    n = kern.run(dA.data_ptr(), dB.data_ptr())
    torch.cuda.synchronize()
    steps = n * _step(opts)
    assert steps >= spec.iterations
    pts = oracle.Spec(stc, ndim, 1).points
    ref = roll_reference(pts, A0[H:-H, H:-H, H:-H], steps)
    got = dA.cpu().numpy()[H:-H, H:-H, H:-H]
    assert _rel(got, ref) <= 1e-12
