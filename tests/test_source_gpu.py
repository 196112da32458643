"""--source (out = S(in) + src; with --time-order 2 (S(in) - out_old) + src) on the MI355X through the C ABI: the small cases of
tests/source_cases.py bit for bit against the host reference (oracle sweep + numpy operations), edge grids, a guard-band arena around
three arrays, the manufactured fixed point, two samples of the tuner's space, full-size C4 / C2 launches (byte offsets past 2^32) and
the emitted --check program.  Every kernel is prebuilt by __graft_entry__.build(): nothing here starts hipcc."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from source_cases import (ARENA, BOTH, CHANNEL_CASE, CHECK_PROGRAM, FIXED_POINT, MIN_CHECKED, PERIODIC_CASE, SAMPLES, SMALL, check_program_path, edge_cases,
                          fixed_point, full_cases, host_launch, host_run, interior, modes_of, sample_jobs, signed_random)

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


def _npdt(opts):
    return np.float32 if "fp32" in opts else np.float64


def _ring(shape, H):
    ring = np.ones(shape, bool)
    ring[tuple(slice(H, s - H) for s in shape)] = False
    return ring


def _check_case(torch, cid, ndim, stc, opts, run=True):
    """One launch: A, B and F bit for bit (F unchanged, out's ring untouched); then the spec's ping-pong run, dr and gold."""
    import drstencil_amd as drs
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    order2 = "--time-order" in opts
    modes = modes_of(opts, ndim)
    assert kern.source and kern.info["stages"] == 1 and kern.time_order == (2 if order2 else 1)
    sz = 4 if "fp32" in opts else 8
    assert kern.bytes_per_launch() == (3 + order2) * sz * int(np.prod(spec.shape)) and kern.array_bytes() == sz * int(np.prod(spec.shape))
    with pytest.raises(ValueError):
        kern.launch(1, 2)                                # a source kernel needs d_src (refused before anything is launched)
    dt = _npdt(opts)
    A0, B0, F0 = (signed_random(spec.shape, dt, s) for s in (11, 12, 13))
    ring = _ring(spec.shape, H)
    dA, dB, dF = (torch.from_numpy(x).cuda() for x in (A0, B0, F0))
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_src=dF.data_ptr())
    torch.cuda.synchronize()
    Ar, Br = A0.copy(), B0.copy()
    host_launch(spec, Ar, Br, F0, modes, order2)
    A1, B1, F1 = dA.cpu().numpy(), dB.cpu().numpy(), dF.cpu().numpy()
    assert np.array_equal(F1, F0), cid
    assert np.array_equal(B1[ring], B0[ring]), cid
    assert np.array_equal(A1, Ar) and np.array_equal(B1, Br), (cid, int((B1 != Br).sum()))
    Bz = B0.copy()
    host_launch(spec, A0.copy(), Bz, np.zeros_like(F0), modes, order2)
    assert not np.array_equal(interior(Bz, H), interior(B1, H))          # the term is seen
    if not run:
        return kern
    Ar, Br = A0.copy(), B0.copy()
    host_run(spec, Ar, Br, F0, spec.launches, modes, order2)
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        n = kern.run(dA.data_ptr(), dB.data_ptr(), gold=gold, d_src=dF.data_ptr())
        torch.cuda.synchronize()
        assert n == spec.launches
        assert np.array_equal(dA.cpu().numpy(), Ar) and np.array_equal(dB.cpu().numpy(), Br), (cid, gold)
        assert np.array_equal(dF.cpu().numpy(), F0), (cid, gold)
    return kern


_SMALL = SMALL + BOTH + [PERIODIC_CASE, CHANNEL_CASE]


@pytest.mark.parametrize("cid,ndim,stc,opts", _SMALL, ids=[c[0] for c in _SMALL])
def test_source_small_vs_host_reference(torch_cuda, cid, ndim, stc, opts):
    _check_case(torch_cuda, cid, ndim, stc, opts)


@pytest.mark.parametrize("cid,ndim,stc,opts", edge_cases(), ids=[c[0] for c in edge_cases()])
def test_source_edge_grids(torch_cuda, cid, ndim, stc, opts):
    """3 x 3 x 3 (one interior cell, element path, fixed and periodic), 7 x 9 x 13 and N = 2 Halo + 257 with branch and buffer masks,
    each under the modest 16-lane geometry and the default one."""
    _check_case(torch_cuda, cid, ndim, stc, opts)


def test_plain_kernel_takes_no_source(torch_cuda):
    import drstencil_amd as drs
    cid, ndim, stc, opts = SMALL[0]
    kern = drs.Kernel([o for o in opts if o != "--source"] + [stc])
    assert not kern.source and kern.bytes_per_launch() == 2 * kern.array_bytes()
    for call in (kern.launch, kern.launch_gold, kern.run, kern.run_timed):
        with pytest.raises(ValueError):
            call(1, 2, d_src=3)
    assert drs.lib().drs_kernel_launch_src(kern.h, 1, 2, 3, 0) == -2       # refused before anything is launched


@pytest.mark.parametrize("cid,ndim,stc,opts", ARENA, ids=[c[0] for c in ARENA])
def test_source_guard_bands(torch_cuda, cid, ndim, stc, opts):
    """Three arrays carved out of one arena at 16-byte alignment with NaN-with-payload guard bands before, between and behind them, the
    same NaN in F's and out's rings: after a launch every guard element, all of in, all of F and out's ring are bit-unchanged and no
    NaN reached out's interior.  An overrun is detected here, never trapped."""
    import drstencil_amd as drs
    from footprint import NAN_BITS, int_view
    torch = torch_cuda
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    tdt = torch.float32 if "fp32" in opts else torch.float64
    n = int(np.prod(spec.shape))
    guard = 4096 + 4                                     # elements: every array 16-byte aligned, none more than that
    step = -(-(guard + n) // 4) * 4
    off = [guard, guard + step, guard + 2 * step]        # in, out, src
    arena = torch.empty(off[2] + n + guard, dtype=tdt, device="cuda")
    poison = NAN_BITS[np.dtype(_npdt(opts))]
    int_view(torch, arena).fill_(poison - (1 << 64) if poison >= (1 << 63) else poison)
    dA, dB, dF = (arena[o:o + n].view(spec.shape) for o in off)
    assert all(t.data_ptr() % 16 == 0 for t in (dA, dB, dF))
    A0 = torch.from_numpy(oracle.fill_random(spec.shape, _npdt(opts))).cuda()
    F0 = torch.from_numpy(oracle.fill_random(spec.shape, _npdt(opts), seed=9)).cuda()
    inner = tuple(slice(H, s - H) for s in spec.shape)
    dA.copy_(A0)
    dF[inner] = F0[inner]
    before = int_view(torch, arena).clone()
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_src=dF.data_ptr())
    torch.cuda.synchronize()
    changed = (before != int_view(torch, arena)).view(-1)
    mask = torch.zeros(spec.shape, dtype=torch.bool, device="cuda")
    mask[inner] = True
    allowed = torch.zeros_like(changed)
    allowed[off[1]:off[1] + n] = mask.view(-1)
    assert not bool((changed & ~allowed).any()), "%s: %d elements outside out's interior were written" % (cid, int((changed & ~allowed).sum()))
    assert not bool(torch.isnan(dB[inner]).any()), cid
    Br = np.zeros(spec.shape, _npdt(opts))
    host_launch(spec, A0.cpu().numpy(), Br, F0.cpu().numpy())
    assert np.array_equal(dB[inner].cpu().numpy(), Br[inner]), cid


def test_fixed_point_fp64(torch_cuda):
    """t3_star fp64: F = u* - S(u*) computed by numpy shifted slices; one launch from in = u* returns u* on the interior within 1e-12
    (the roundings of one chain and one add).  No oracle involved."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = FIXED_POINT
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, 1)
    u, F = fixed_point(spec)
    dA, dF = torch.from_numpy(u).cuda(), torch.from_numpy(F).cuda()
    dB = torch.zeros_like(dA)
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_src=dF.data_ptr())
    torch.cuda.synchronize()
    err = float(np.max(np.abs(interior(dB.cpu().numpy(), spec.halo) - interior(u, spec.halo))))
    print("fixed point: max abs error %.3g" % err)
    assert err <= 1e-12, err


@pytest.mark.parametrize("which", list(SAMPLES))
def test_source_sampled_space(torch_cuda, which):
    """The sample of 20 against the host reference (one launch and the spec's run, dr and gold); kernels the runtime or the generator
    refused when build() compiled are not in the cache and are counted: at least three quarters checked."""
    import drstencil_amd as drs
    checked = 0
    for ndim, stc, dtype, args, step in sample_jobs(which):
        try:
            drs.Kernel(args)
        except drs.KernelBuildError:
            continue
        _check_case(torch_cuda, "%s %s" % (which, " ".join(args[:-1])), ndim, stc, args[:-1])
        checked += 1
    print("%s: %d of 20 checked" % (which, checked))
    assert checked >= MIN_CHECKED, (which, checked)


@pytest.mark.parametrize("case", [0, 1], ids=["C4_step1", "C2_step1"])
def test_full_size_source_launch(torch_cuda, case):
    """BASELINE sizes, one launch, the tuned step-1 row + --source: dr == gold on the whole grid, and three slabs (bottom, across a
    stream-block boundary, top: byte offsets past 2^32 in 3D) against the oracle composed with F's slabs."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = full_cases()[case]
    kern = drs.Kernel(opts + [stc])
    i = kern.info
    H = i["halo"]
    assert kern.source and kern.time_order == 1 and i["arithmetic"] == "gold-order"
    shape = (i["L"], i["M"], i["N"]) if ndim == 3 else (i["M"], i["N"])
    assert kern.bytes_per_launch() == 3 * 4 * int(np.prod(shape))
    g = torch.Generator(device="cuda").manual_seed(1234)
    A = torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)
    F = torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)
    B0 = torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)
    B, Bg = B0.clone(), B0.clone()
    kern.launch(A.data_ptr(), B.data_ptr(), d_src=F.data_ptr())
    kern.launch_gold(A.data_ptr(), Bg.data_ptr(), d_src=F.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(B, Bg), cid
    del Bg
    ring = torch.ones(shape, dtype=torch.bool, device="cuda")
    ring[tuple(slice(H, s - H) for s in shape)] = False
    assert torch.equal(B[ring], B0[ring]), cid
    del ring
    spec = oracle.Spec(stc, ndim, 1)
    n0, sn, thick = shape[0], i["sn"], 6
    boundary = H + sn * max(1, ((n0 // 2) // sn))              # a stream-block boundary near the middle
    for lo in (0, boundary - thick // 2, n0 - thick):
        a = np.ascontiguousarray(A[lo:lo + thick].cpu().numpy())
        f = np.ascontiguousarray(F[lo:lo + thick].cpu().numpy())
        if ndim == 3:
            spec.set_dims(thick, shape[1], shape[2])
        else:
            spec.set_dims(1, thick, shape[1])
        ref = host_launch(spec, a, np.ascontiguousarray(B0[lo:lo + thick].cpu().numpy()), f)      # out's ring keeps what it held
        got = B[lo:lo + thick].cpu().numpy()
        assert np.array_equal(got[H:-H], ref[H:-H]), (cid, lo)      # the slab's own outer planes / rows are not recomputed


def test_emitted_check_program(torch_cuda):
    """The standalone program emitted with --check --source (built by build()): dr_ and gold_ run the same launch sequence from
    identical copies of (A, B) with the same src; the check reports no difference."""
    exe = check_program_path()
    assert os.path.exists(exe), "build() has not built %s" % exe
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, out[-1500:] + p.stderr[-500:]
    assert "[Test] RMS Error: 0.000000e+00" in out and "differ" not in out, out[-1500:]
    assert CHECK_PROGRAM[0]
