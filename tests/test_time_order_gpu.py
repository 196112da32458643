"""--time-order 2 (out = S(in) - out_old) on the MI355X through the C ABI: the small cases of tests/wave_cases.py bit for bit against
the host reference (oracle sweep + one subtraction), periodic + order 2, the analytic plane wave, dr == gold, untouched rings, a
guard-band arena, full-size C4 / C2 launches (byte offsets past 2^32) and the emitted --check program.  Every kernel is prebuilt by
__graft_entry__.build(): nothing here starts hipcc."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from wave_cases import ARENA, CHECK_PROGRAM, PERIODIC_CASE, PLANE_WAVE, SMALL, check_program_path, full_cases, host_launch, host_run, interior, plane_wave

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


@pytest.mark.parametrize("cid,ndim,stc,opts", SMALL + [PERIODIC_CASE], ids=[c[0] for c in SMALL + [PERIODIC_CASE]])
def test_order_2_small_vs_host_reference(torch_cuda, cid, ndim, stc, opts):
    """Kernel.run for the spec's iterations from random A and random B: both arrays bit for bit, dr == gold, out's ring untouched
    (periodic: in's ring wrapped, out's unchanged after one launch)."""
    import drstencil_amd as drs
    torch = torch_cuda
    periodic = "periodic" in opts
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    assert kern.time_order == 2 and kern.info["stages"] == 1 and kern.periodic == periodic
    sz = 4 if "fp32" in opts else 8
    assert kern.bytes_per_launch() == 3 * sz * int(np.prod(spec.shape)) and kern.array_bytes() * 3 == kern.bytes_per_launch()
    assert kern.updates_per_launch() == int(np.prod([d - 2 * H for d in spec.shape]))
    A0 = oracle.fill_random(spec.shape, _npdt(opts))
    B0 = oracle.fill_random(spec.shape, _npdt(opts), seed=9)
    ring = _ring(spec.shape, H)
    # one launch
    dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
    kern.launch(dA.data_ptr(), dB.data_ptr())
    torch.cuda.synchronize()
    Ar, Br = A0.copy(), B0.copy()
    host_launch(spec, Ar, Br, periodic)
    A1, B1 = dA.cpu().numpy(), dB.cpu().numpy()
    assert np.array_equal(B1[ring], B0[ring]), cid
    assert np.array_equal(A1, Ar) and np.array_equal(B1, Br), cid
    assert not np.array_equal(interior(B1, H), interior(B0, H))
    # the spec's ping-pong run, dr and gold
    Ar, Br = A0.copy(), B0.copy()
    host_run(spec, Ar, Br, spec.launches, periodic)
    for gold in (False, True):
        dA, dB = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        n = kern.run(dA.data_ptr(), dB.data_ptr(), gold=gold)
        torch.cuda.synchronize()
        assert n == spec.launches
        assert np.array_equal(dA.cpu().numpy(), Ar) and np.array_equal(dB.cpu().numpy(), Br), (cid, gold)


def test_plane_wave_fp64(torch_cuda):
    """t3_wave periodic fp64: u(t) = cos(k.x - w t) solves the leapfrog recurrence exactly; after the spec's 8 launches the array
    written last equals cos(k.x - 8 w) within 1e-12 (only rounding is left).  No oracle involved."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = PLANE_WAVE
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, 1)
    A, B, exact = plane_wave(spec.shape, spec.halo, spec.points)
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    assert kern.run(dA.data_ptr(), dB.data_ptr()) == 8
    torch.cuda.synchronize()
    err = float(np.max(np.abs(interior(dA.cpu().numpy(), 1) - exact(8))))
    print("plane wave after 8 launches: max abs error %.3g" % err)
    assert err <= 1e-12, err
    assert float(np.max(np.abs(interior(dB.cpu().numpy(), 1) - exact(7)))) <= 1e-12


@pytest.mark.parametrize("cid,ndim,stc,opts", ARENA, ids=[c[0] for c in ARENA])
def test_order_2_guard_bands(torch_cuda, cid, ndim, stc, opts):
    """Both arrays inside one arena at 16-byte alignment, NaN-with-payload guard bands before, between and behind them and in out's
    ring: after a launch every guard byte and out's ring are bit-unchanged, in is unchanged and no NaN reached out's interior.  An
    overrun is detected here, never provoked."""
    import drstencil_amd as drs
    from footprint import NAN_BITS, int_view
    torch = torch_cuda
    kern = drs.Kernel(opts + [stc])
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    tdt = torch.float32 if "fp32" in opts else torch.float64
    n = int(np.prod(spec.shape))
    guard = 4096 + 4                                     # elements: both arrays 16-byte aligned, neither more than that
    off_b = -(-(2 * guard + n) // 4) * 4                 # the output's first element
    arena = torch.empty(off_b + n + guard, dtype=tdt, device="cuda")
    poison = NAN_BITS[np.dtype(_npdt(opts))]
    int_view(torch, arena).fill_(poison - (1 << 64) if poison >= (1 << 63) else poison)
    dA = arena[guard:guard + n].view(spec.shape)
    dB = arena[off_b:off_b + n].view(spec.shape)
    assert dA.data_ptr() % 16 == 0 and dB.data_ptr() % 16 == 0
    A0 = torch.from_numpy(oracle.fill_random(spec.shape, _npdt(opts))).cuda()
    B0 = torch.from_numpy(oracle.fill_random(spec.shape, _npdt(opts), seed=9)).cuda()
    inner = tuple(slice(H, s - H) for s in spec.shape)
    dA.copy_(A0)
    dB[inner] = B0[inner]
    before = int_view(torch, arena).clone()
    kern.launch(dA.data_ptr(), dB.data_ptr())
    torch.cuda.synchronize()
    after = int_view(torch, arena)
    changed = (before != after).view(-1)
    mask = torch.zeros(spec.shape, dtype=torch.bool, device="cuda")
    mask[inner] = True
    allowed = torch.zeros_like(changed)
    allowed[off_b:off_b + n] = mask.view(-1)
    assert not bool((changed & ~allowed).any()), "%s: %d elements outside out's interior were written" % (cid, int((changed & ~allowed).sum()))
    assert not bool(torch.isnan(dB[inner]).any()), cid
    Br = B0.cpu().numpy()
    host_launch(spec, A0.cpu().numpy(), Br)
    assert np.array_equal(dB[inner].cpu().numpy(), Br[inner]), cid


@pytest.mark.parametrize("case", [0, 1], ids=["C4_step1", "C2_step1"])
def test_full_size_order_2_launch(torch_cuda, case):
    """BASELINE sizes, one launch, the tuned step-1 row + --time-order 2: dr == gold on the whole grid, and three slabs (bottom, across a
    stream-block boundary, top: byte offsets past 2^32 in 3D) against the oracle composed with the old values of those slabs."""
    import drstencil_amd as drs
    torch = torch_cuda
    cid, ndim, stc, opts = full_cases()[case]
    kern = drs.Kernel(opts + [stc])
    i = kern.info
    H = i["halo"]
    assert kern.time_order == 2 and i["arithmetic"] == "gold-order"
    shape = (i["L"], i["M"], i["N"]) if ndim == 3 else (i["M"], i["N"])
    assert kern.bytes_per_launch() == 3 * 4 * int(np.prod(shape))
    g = torch.Generator(device="cuda").manual_seed(1234)
    A = torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)
    B0 = torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)
    B, Bg = B0.clone(), B0.clone()
    kern.launch(A.data_ptr(), B.data_ptr())
    kern.launch_gold(A.data_ptr(), Bg.data_ptr())
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
        old = np.ascontiguousarray(B0[lo:lo + thick].cpu().numpy())
        if ndim == 3:
            spec.set_dims(thick, shape[1], shape[2])
        else:
            spec.set_dims(1, thick, shape[1])
        ref = host_launch(spec, a, old.copy())
        got = B[lo:lo + thick].cpu().numpy()
        assert np.array_equal(got[H:-H], ref[H:-H]), (cid, lo)      # the slab's own outer planes / rows are not recomputed


def test_emitted_check_program(torch_cuda):
    """The standalone program emitted with --check --time-order 2 (built by build()): dr_ and gold_ run the same launch sequence from
    identical copies of (A, B), both restored after the warm-up; the check reports no difference."""
    exe = check_program_path()
    assert os.path.exists(exe), "build() has not built %s" % exe
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, out[-1500:] + p.stderr[-500:]
    assert "[Test] RMS Error: 0.000000e+00" in out and "differ" not in out, out[-1500:]
    assert "[Test] Max Error : 1.000000e-13" in out, out[-1500:]
    assert CHECK_PROGRAM[0]
