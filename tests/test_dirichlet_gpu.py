"""--dirichlet on the MI355X through the C ABI: the case list of tests/dirichlet_cases.py (the one tests/test_dirichlet_cpu.py runs under
the emulation) -- three launches each of dr_ and of gold_, whole arrays bit for bit against the job's host reference followed by np.where
on the interior --, planted held cells and their complement, all free against the same command without the option, all held, NaN markers
of every kind with held values arithmetic would not keep, a guard-band arena, the samples of the tuner's space, the residual of every mode,
the run to tolerance around held cells (drs_kernel_solve_fix) and the emitted --check program.
Every kernel is prebuilt by __graft_entry__.build(): nothing here starts hipcc.  The references are computed on the host once per test."""
import os
import subprocess

import numpy as np
import pytest

import dirichlet_cases as dc
import oracle
import residual_cases as rc
from footprint import bit_equal
from special_values import count_different, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


def _kernel(opts, stc):
    import drstencil_amd as drs
    return drs.Kernel(dc.with_fix(opts) + [stc])


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(a).cuda() for a in arrays]


def _kw(dF, dR, dX):
    kw = {"d_fix": dX.data_ptr()}
    if dF is not None:
        kw["d_src"] = dF.data_ptr()
    if dR is not None:
        kw["d_res"] = dR.data_ptr()
    return kw


def _nan_res(torch, kern, dt):
    if not kern.residual_elems:
        return None
    return torch.full((kern.residual_elems,), float("nan"), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")


def _launches(torch, kern, spec, ndim, opts, A0, B0, F0, X, what, launches=3, gold=False):
    """`launches` launches from (A0, B0, F0) with held cells X: after each, both WHOLE arrays equal the host reference's in bits; with
    --residual max r equals numpy's in bits and every element of the NaN-filled residual array has been overwritten."""
    dt = A0.dtype
    dA, dB, dF, dX = _dev(torch, A0, B0, F0, X)
    Ar, Br = A0.copy(), B0.copy()
    for t in range(launches):
        s, d = (dA, dB) if t % 2 == 0 else (dB, dA)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        dR = None if gold else _nan_res(torch, kern, dt)
        if gold:
            kern.launch_gold(s.data_ptr(), d.data_ptr(), **_kw(dF, None, dX))
        else:
            kern.launch(s.data_ptr(), d.data_ptr(), **_kw(dF, dR, dX))
        torch.cuda.synchronize()
        want = dc.host_launch(spec, ndim, opts, sr, dr, F0, X)
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        assert same_bits(A, Ar) and same_bits(B, Br), (what, t, count_different(A, Ar), count_different(B, Br))
        if dR is not None:
            R = dR.cpu().numpy()
            print(what, "launch", t, "r", repr(R[0]), "reference", repr(want))
            assert rc.same_bits(R[0], want), (what, t, R[0], want)
            assert not np.isnan(R).any() or np.isnan(want), (what, t, "partials not written")
    assert bit_equal(dX.cpu().numpy(), X) and (F0 is None or bit_equal(dF.cpu().numpy(), F0)), (what, "fix or src was written")
    return dA.cpu().numpy(), dB.cpu().numpy()


# ---- 1. bit-exactness -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_dirichlet_cases(torch_cuda, cid, ndim, stc, opts):
    kern = _kernel(opts, stc)
    assert kern.dirichlet and kern.info["dirichlet"] == 1 and kern.info["stages"] == 1
    assert kern.resources.get("scratch_bytes_per_lane", 0) == 0 and kern.resources.get("sgpr_spill", 0) == 0
    if cid == dc.BIG[0]:
        assert kern.info["stream_blocks"] == 9 and kern.info["tiles_x"] * kern.info["tiles_y"] == 18 and kern.info["grid"] == 168
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X = dc.inputs(spec, opts)
    if cid == dc.MIN_333[0]:
        for v in (0.375, np.nan):                       # one interior cell: once held, once free
            X[1, 1, 1] = v
            _launches(torch_cuda, kern, spec, ndim, opts, A0, B0, F0, X, (cid, v))
            _launches(torch_cuda, kern, spec, ndim, opts, A0, B0, F0, X, (cid, v, "gold"), gold=True)
        return
    held, free = dc.held_and_free(X, spec.halo)
    assert held >= 1 and free >= 1, (cid, held, free)                      # on the pattern alone
    _launches(torch_cuda, kern, spec, ndim, opts, A0, B0, F0, X, cid)
    _launches(torch_cuda, kern, spec, ndim, opts, A0, B0, F0, X, (cid, "gold"), gold=True)


# ---- 2. planted cells -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", dc.PLANT, ids=[c[0] for c in dc.PLANT])
def test_planted_cells(torch_cuda, cid, ndim, stc, opts):
    """Held: exactly the interior corners and both sides of every x, y and z seam; then exactly their complement."""
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, _ = dc.inputs(spec, opts)
    cells = rc.planted_cells(kern.info)
    assert len(cells) >= (14 if cid.startswith(dc.BIG[0]) else 10), (cid, len(cells))
    vals = dc.fix_pattern(spec.shape, A0.dtype, 5)
    vals[np.isnan(vals)] = 0.625
    planted = np.zeros(spec.shape, bool)
    for c in cells:
        planted[c] = True
    I = tuple(slice(spec.halo, n - spec.halo) for n in spec.shape)
    for mask in (planted, ~planted):
        X = np.where(mask, vals, np.asarray(np.nan, A0.dtype)).astype(A0.dtype)
        A, B = _launches(torch_cuda, kern, spec, ndim, opts, A0, B0, F0, X, (cid, int(mask.sum())), launches=2)
        assert np.array_equal(B[I][mask[I]], vals[I][mask[I]]) and not np.array_equal(B[I][~mask[I]], vals[I][~mask[I]])


# ---- 3. all free, all held ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", dc.UNCHANGED, ids=[c[0] for c in dc.UNCHANGED])
def test_all_free_and_all_held(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    from footprint import nan_filled
    torch = torch_cuda
    kern = _kernel(opts, stc)
    plain = drs.Kernel(list(opts) + [stc])
    assert not plain.dirichlet and "dirichlet" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    A0, B0, F0, X = dc.inputs(spec, opts)
    X[...] = np.nan
    dA1, dB1, dF, dX = _dev(torch, A0, B0, F0, X)
    dA2, dB2 = _dev(torch, A0, B0)
    src = {"d_src": dF.data_ptr()} if dF is not None else {}
    for t in range(2):
        a, b = ((dA1, dB1), (dB1, dA1))[t]
        kern.launch(a.data_ptr(), b.data_ptr(), **_kw(dF, None, dX))
        a, b = ((dA2, dB2), (dB2, dA2))[t]
        plain.launch(a.data_ptr(), b.data_ptr(), **src)
        torch.cuda.synchronize()
        assert bit_equal(dA1.cpu().numpy(), dA2.cpu().numpy()) and bit_equal(dB1.cpu().numpy(), dB2.cpu().numpy()), (cid, t)
    # all held: `in` entirely NaN, the output's interior is fix's, its ring and all of `in` are bit-unchanged
    assert "--boundary" not in opts
    Xall = rc.inputs(spec, opts, 31)[0]
    Anan = nan_filled(spec.shape, A0.dtype)
    dA, dB, dX = _dev(torch, Anan, B0, Xall)
    kern.launch(dA.data_ptr(), dB.data_ptr(), **_kw(dF, None, dX))
    torch.cuda.synchronize()
    want = B0.copy()
    rc.interior(want, H)[...] = rc.interior(Xall, H)
    assert bit_equal(dA.cpu().numpy(), Anan) and bit_equal(dB.cpu().numpy(), want), cid


# ---- 4. sentinels and special values --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", dc.PLANT, ids=[c[0] for c in dc.PLANT])
def test_special_values(torch_cuda, cid, ndim, stc, opts):
    """Free cells marked by NaNs of both signs, quiet and signalling, with payloads; held values +0.0, -0.0, the smallest subnormals and
    +-inf; NaN, inf and -0.0 planted in `in` so that a select and a blend m * v + (1 - m) * fix differ (dirichlet_cases.special_problem).
    The four built conditions are asserted on the reference alone."""
    torch = torch_cuda
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, cells = dc.special_problem(spec, opts)
    Ar, Br = A0.copy(), B0.copy()
    unheld = np.zeros_like(A0)
    dc.host_launch(spec, ndim, opts, Ar, Br, F0, X, unheld=unheld)
    m0 = np.asarray(-0.0, A0.dtype).tobytes()
    assert not np.isnan(X[cells["held_nan"]]) and np.isnan(unheld[cells["held_nan"]])
    assert not np.isnan(X[cells["held_inf"]]) and np.isinf(unheld[cells["held_inf"]])
    assert np.isnan(X[cells["free_nan"]]) and np.isnan(Br[cells["free_nan"]])
    assert np.isnan(X[cells["free_m0"]]) and Br[cells["free_m0"]].tobytes() == m0
    Ar2, Br2 = Ar.copy(), Br.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        dc.host_launch(spec, ndim, opts, Br2, Ar2, F0, X)
    for gold in (False, True):
        dA, dB, dF, dX = _dev(torch, A0, B0, F0, X)
        fn = kern.launch_gold if gold else kern.launch
        fn(dA.data_ptr(), dB.data_ptr(), **_kw(dF, None, dX))
        torch.cuda.synchronize()
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        assert same_bits(A, Ar) and same_bits(B, Br), (cid, gold, count_different(B, Br))
        fn(dB.data_ptr(), dA.data_ptr(), **_kw(dF, None, dX))       # the second launch carries the held infinities and the NaNs through the sweep
        torch.cuda.synchronize()
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        assert same_bits(A, Ar2) and same_bits(B, Br2), (cid, gold, count_different(A, Ar2))


# ---- 5. memory contract: a guard-band arena -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", dc.ARENA, ids=[c[0] for c in dc.ARENA])
def test_dirichlet_guard_bands(torch_cuda, cid, ndim, stc, opts):
    """in, out and fix carved out of one arena between NaN-with-payload guard bands; fix's ring is NaN-free garbage.  After a launch
    every guard element, all of `in` and all of fix are bit-unchanged, out's ring too.  An overrun is detected here, never trapped."""
    from footprint import NAN_BITS, int_view, ring_mask
    torch = torch_cuda
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    dt = dc.dtype_of(opts)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    n = int(np.prod(spec.shape))
    guard = 4096 + 4                                     # elements: every array 16-byte aligned, none more than that
    step = -(-(guard + n) // 4) * 4
    off = [guard, guard + step, guard + 2 * step]        # in, out, fix
    total = off[2] + n + guard
    arena = torch.empty(total, dtype=tdt, device="cuda")
    int_view(torch, arena).fill_(NAN_BITS[np.dtype(dt)])
    before = int_view(torch, arena).clone()
    A0, B0, _, X = dc.inputs(spec, opts)
    ring = ring_mask(spec.shape, H)
    X[ring] = (1e30 * (1 + np.arange(int(ring.sum())) % 7)).astype(dt)
    dA = arena[off[0]:off[0] + n].view(spec.shape)
    dB = arena[off[1]:off[1] + n].view(spec.shape)
    dX = arena[off[2]:off[2] + n].view(spec.shape)
    dA.copy_(torch.from_numpy(A0))
    dX.copy_(torch.from_numpy(X))
    inner = tuple(slice(H, s - H) for s in spec.shape)
    dB[inner] = torch.from_numpy(np.ascontiguousarray(B0[inner])).cuda()
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_fix=dX.data_ptr())
    torch.cuda.synchronize()
    after = int_view(torch, arena)
    keep = torch.ones(total, dtype=torch.bool, device="cuda")
    for o in off:
        keep[o:o + n] = False
    assert torch.equal(after[keep], before[keep]), (cid, "a guard band was written")
    assert bit_equal(dA.cpu().numpy(), A0) and bit_equal(dX.cpu().numpy(), X), cid
    Br = B0.copy()
    dc.host_launch(spec, ndim, opts, A0.copy(), Br, None, X)
    Bg = dB.cpu().numpy()
    assert np.isnan(Bg[ring]).all() and bit_equal(np.ascontiguousarray(Bg[inner]), np.ascontiguousarray(Br[inner])), cid


# ---- 6. the samples of the tuner's space ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(dc.SAMPLES))
def test_dirichlet_sampled_fuzz(torch_cuda, which):
    """A seeded sample of the tuner's space: every member that build() compiled, three launches each; at least three quarters of the
    sample are checked (the refusals were decided by the generator and the compiler)."""
    import drstencil_amd as drs
    checked = 0
    for n, (ndim, path, dtype, args, step) in enumerate(dc.sample_jobs(which)):
        try:
            kern = drs.Kernel(args)
        except drs.KernelBuildError:
            continue
        spec = oracle.Spec(path, ndim, step)
        A0, B0, F0, X = dc.inputs(spec, args[:-1])
        _launches(torch_cuda, kern, spec, ndim, args[:-1], A0, B0, F0, X, "%s %02d" % (which, n))
        checked += 1
    assert checked >= dc.MIN_CHECKED, checked


# ---- 7. residual and run to tolerance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", dc.RES_MODES[:-1], ids=[c[0] for c in dc.RES_MODES[:-1]])
def test_residual_with_held_cells(torch_cuda, cid, ndim, stc, opts):
    """r = np.max(np.abs(out_I - in_I)) in bits after every launch, held cells included (the last of RES_MODES runs in test_dirichlet_cases)."""
    kern = _kernel(opts, stc)
    assert kern.residual_elems == 1 + kern.info["grid"] and kern.dirichlet
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X = dc.inputs(spec, opts)
    _launches(torch_cuda, kern, spec, ndim, opts, A0, B0, F0, X, cid)


_SOLVE = [(c[0] + "_" + k, c[1], c[2], c[3], c[4], k) for c in dc.SOLVE for k in dc.SOLVE_KINDS]


@pytest.mark.parametrize("cid,ndim,stc,opts,tol,kind", _SOLVE, ids=[c[0] for c in _SOLVE])
def test_run_to_tolerance(torch_cuda, cid, ndim, stc, opts, tol, kind):
    """jacobi3 on 18^3 with a ring of 0: an inner block held at 1.0, and an octant held at 0 (an L-shaped domain).  Kernel.solve
    (drs_kernel_solve_fix) returns the status, the launch count and the r of a numpy loop of oracle sweeps with the np.where after each that
    looks at r at the same launches; held cells are bit-exactly their values in A and B; every value lies in [0, 1]."""
    torch = torch_cuda
    kern = _kernel(opts + rc.RES, stc)
    spec = oracle.Spec(stc, ndim, 1)
    dt = dc.dtype_of(opts)
    A, B, X = dc.solve_problem(spec, dt, kind)
    Ar, Br = A.copy(), B.copy()
    want = dc.oracle_solve(spec, Ar, Br, None, X, tol, dc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and want[1] < dc.MAX_LAUNCHES and want[1] % 8 == 0, want
    dA, dB, dX = _dev(torch, A, B, X)
    dR = _nan_res(torch, kern, dt)
    status, launches, r = kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), tol, dc.MAX_LAUNCHES, check_every=4, d_fix=dX.data_ptr())
    print(cid, "launches", launches, "residual", repr(r), "reference", want)
    assert status == 0 and launches == want[1], (status, launches, want)
    assert rc.same_bits(np.asarray(r, dt), want[2]) and kern.residual(dR.data_ptr()) == r
    Ag, Bg = dA.cpu().numpy(), dB.cpu().numpy()
    assert bit_equal(Ag, Ar) and bit_equal(Bg, Br)
    held = ~np.isnan(X)
    assert bit_equal(Ag[held], X[held]) and bit_equal(Bg[held], X[held])
    assert Ag.min() >= 0.0 and Ag.max() <= 1.0 and Bg.min() >= 0.0 and Bg.max() <= 1.0
    # max_launches = 16: status 1 with 16 launches; run() and run_timed(): the reference's loop with held cells
    dA, dB = _dev(torch, A, B)
    assert kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), tol, 16, check_every=4, d_fix=dX.data_ptr())[:2] == (1, 16)
    dA, dB = _dev(torch, A, B)
    n = kern.run(dA.data_ptr(), dB.data_ptr(), iterations=8, d_res=dR.data_ptr(), d_fix=dX.data_ptr())
    Ar, Br = A.copy(), B.copy()
    ref = dc.oracle_solve(spec, Ar, Br, None, X, 0.0, 8, 4)
    assert n == 8 and rc.same_bits(np.asarray(kern.residual(dR.data_ptr()), dt), ref[2]) and bit_equal(dA.cpu().numpy(), Ar)
    n, ms = kern.run_timed(dA.data_ptr(), dB.data_ptr(), iterations=4, warmup=0, d_res=dR.data_ptr(), d_fix=dX.data_ptr())
    assert n == 4 and ms > 0
    dc.oracle_solve(spec, Ar, Br, None, X, 0.0, 4, 2)
    assert bit_equal(dA.cpu().numpy(), Ar)


# ---- 8. interface -------------------------------------------------------------------------------------------------------------------
def test_emitted_check_program(torch_cuda):
    """The prebuilt --check --dirichlet program (periodic, order 2, source, residual): dr_ and gold_ run with the same fix and agree."""
    exe = dc.check_program_path()
    assert os.path.exists(exe), "build() makes it"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, (p.returncode, out[-1500:], p.stderr[-500:])
    assert "residual : " in out and "[Test] RMS Error: 0.000000e+00" in out and "[Test] Residual Error: 0.000000e+00" in out and "differ" not in out, out[-1500:]
