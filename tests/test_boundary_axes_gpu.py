"""--boundary reflect and --boundary-x / -y / -z on the MI355X: the ring-fill kernel against boundary_cases.host_fill and sweeps
against the CPU oracle with that fill in front of every launch (bit for bit for single-pass kernels, within 1e-6 fp32 / 1e-12 fp64 for
on-chip temporal pipelines) on the edge grids, on the reflect and mixed variants of five seeded cases, on a sample of the tuner's
space and at full size (C4, 1024^3: byte offsets past 2^32).  Every kernel is prebuilt by __graft_entry__.build()
(tests/boundary_cases.py): nothing here starts hipcc."""
import numpy as np
import pytest

import boundary_cases as bc
import fuzz_parity
import oracle
from boundary_cases import fill_destinations, host_fill, oracle_boundary_run

pytestmark = pytest.mark.gpu
REL_TOL = {"fp32": 1e-6, "fp64": 1e-12}
LAUNCHES = 3


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


def _check(torch, kern, ndim, stc, opts, launches=LAUNCHES):
    """wrap() of random A against host_fill, then `launches` launches of dr and of gold from random A and B in [-1, 1) (non-negative
    for pipelines) against oracle_boundary_run; the array filled last is its own host fill; what no fill and no sweep may write is
    bit-unchanged."""
    dt = _dtype(opts)
    modes = bc.modes_of(opts + [stc], ndim)
    assert kern.boundaries == modes and kern.fills_ring and kern.periodic == all(m == "periodic" for m in modes)
    spec = oracle.Spec(stc, ndim, _step(opts))
    H = spec.halo
    assert kern.info["halo"] == H
    temporal = kern.info.get("stages", 1) > 1
    order2 = kern.time_order == 2
    A0, B0 = fuzz_parity.mode_inputs(spec, dt, temporal)
    dest = fill_destinations(A0.shape, H, modes)
    frozen = fuzz_parity.ring_mask(A0.shape, H) & ~dest
    dA = torch.from_numpy(A0).cuda()
    kern.wrap(dA.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dA.cpu().numpy(), host_fill(A0.copy(), H, modes))
    Ar, Br = A0.copy(), B0.copy()
    assert oracle_boundary_run(spec, Ar, Br, modes, launches, order2=order2) == launches
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        for i in range(launches):
            s, d = (dA, dB) if i % 2 == 0 else (dB, dA)
            (kern.launch_gold if gold else kern.launch)(s.data_ptr(), d.data_ptr())
        torch.cuda.synchronize()
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        assert np.array_equal(A[frozen], A0[frozen]) and np.array_equal(B[frozen], B0[frozen]), gold
        filled = A if launches % 2 else B
        assert np.array_equal(filled, host_fill(filled.copy(), H, modes)), gold
        if temporal and not gold:
            rel = max(fuzz_parity.rel_error(A, Ar), fuzz_parity.rel_error(B, Br))
            assert rel <= REL_TOL[dt], rel
        else:
            assert np.array_equal(A, Ar) and np.array_equal(B, Br), (gold, int((A != Ar).sum()), int((B != Br).sum()))


EDGE = bc.edge_cases()


@pytest.mark.parametrize("cid,ndim,stc,opts", EDGE, ids=[c[0] for c in EDGE])
def test_boundary_edge_grids(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    _check(torch_cuda, drs.Kernel(opts + [stc]), ndim, stc, opts)


SMALL = bc.gpu_small_cases()


@pytest.mark.parametrize("cid,ndim,stc,opts", SMALL, ids=[c[0] for c in SMALL])
def test_boundary_small_vs_oracle_with_fill(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    kern = drs.Kernel(opts + [stc])
    assert (kern.info.get("stages", 1) > 1) == ("--temporal" in opts)
    _check(torch_cuda, kern, ndim, stc, opts)


def test_boundary_sampled_fuzz(torch_cuda):
    """The 20 configurations of boundary_cases.sample_jobs, each with its per-axis triple: at least 15 checked; the others are the
    refusals build() reported (spills, LDS-DMA staging on a row length that is no multiple of the vector)."""
    import drstencil_amd as drs
    jobs = bc.sample_jobs()
    assert len(jobs) == bc.SAMPLE[0] == 20
    checked, refused = 0, []
    for ndim, stc, dtype, args, step in jobs:
        try:
            kern = drs.Kernel(args)
        except drs.KernelBuildError as e:
            assert "not in the cache" not in str(e), str(e)           # every kernel of the sample was built, or refused, by build()
            refused.append(" ".join(args[:-1]))
            continue
        _check(torch_cuda, kern, ndim, stc, args[:-1])
        checked += 1
    print("boundary fuzz: %d checked, %d refused" % (checked, len(refused)))
    assert checked >= bc.MIN_CHECKED, (checked, refused)


def test_full_size_c4_reflect(torch_cuda):
    """C4 headline options with rigid walls at 1024^3 fp32 (4 GiB: the top ghost planes lie past 2^32 bytes): wrap() of a random
    array against host_fill on the whole ring, then one launch against the oracle on the three check_slabs slabs."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = bc.full_case()
    kern = drs.Kernel(opts + [stc])
    i = kern.info
    H = i["halo"]
    assert kern.boundaries == ("reflect",) * 3 and i["arithmetic"] == "gold-order"
    g = torch.Generator(device="cuda").manual_seed(4321)
    A = torch.rand((i["L"], i["M"], i["N"]), dtype=torch.float32, device="cuda", generator=g)
    a = A.cpu().numpy()
    kern.wrap(A.data_ptr())
    torch.cuda.synchronize()
    host_fill(a, H, ("reflect",) * 3)
    got = A.cpu().numpy()
    for ax in range(3):                                   # the whole ring, face by face (views: no mask of a billion cells)
        for s in (slice(0, H), slice(-H, None)):
            idx = tuple(s if d == ax else slice(None) for d in range(3))
            assert np.array_equal(got[idx], a[idx]), (ax, s)
    assert np.array_equal(got[H:-H, H:-H, H], a[H:-H, H:-H, H]) and np.array_equal(got[-H - 1], a[-H - 1])      # interior faces stay
    del got
    B = torch.zeros_like(A)
    kern.launch(A.data_ptr(), B.data_ptr())
    torch.cuda.synchronize()
    nsl = 16
    for label, z0 in kern.check_slabs(nsl):
        src = np.ascontiguousarray(a[z0:z0 + nsl])              # the filled input: the bottom and top slabs hold mirrored ghost planes
        ref = np.zeros_like(src)
        cs = oracle.Spec(stc, ndim, _step(opts))
        cs.set_dims(nsl, i["M"], i["N"])
        oracle.sweep(cs, src, ref, contract=1)
        assert np.array_equal(B[z0 + H:z0 + nsl - H].cpu().numpy(), ref[H:nsl - H]), label
