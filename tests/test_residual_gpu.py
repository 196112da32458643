"""--residual max on the MI355X through the C ABI: the case list of tests/residual_cases.py (the one tests/test_residual_cpu.py runs under
the emulation) -- three launches each, arrays bit for bit against the job's host reference and r bit for bit against numpy's
max(abs(out - in)) --, the planted maximum, poisoned inputs with a NaN-filled residual array, special values, a guard-band arena, the
arrays against those of the same command without the option, the run to tolerance (drs_kernel_solve) and the emitted --check program.
Every kernel is prebuilt by __graft_entry__.build(): nothing here starts hipcc.  The references are computed on the host once per test."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import residual_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


def _kernel(opts, stc):
    import drstencil_amd as drs
    return drs.Kernel(rc.with_res(opts) + [stc])


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(a).cuda() for a in arrays]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan_res(torch, kern, dt):
    return torch.full((kern.residual_elems,), float("nan"), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")


def _launch(torch, kern, dS, dD, dF, dt):
    """One launch with a NaN-filled residual array: (r as a 0-d numpy value of the dtype, the whole residual array on the host)."""
    dR = _nan_res(torch, kern, dt)
    kern.launch(dS.data_ptr(), dD.data_ptr(), **({"d_src": _ptr(dF)} if dF is not None else {}), d_res=dR.data_ptr())
    torch.cuda.synchronize()
    R = dR.cpu().numpy()
    return R[0], R


def _three_launches(torch, kern, spec, ndim, opts, A0, B0, F0, what):
    dt = A0.dtype
    dA, dB, dF = _dev(torch, A0, B0, F0)
    Ar, Br = A0.copy(), B0.copy()
    for t in range(3):
        s, d = (dA, dB) if t % 2 == 0 else (dB, dA)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        r, R = _launch(torch, kern, s, d, dF, dt)
        want = rc.host_launch(spec, ndim, opts, sr, dr, F0)
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        print(what, "launch", t, "r", repr(r), "reference", repr(want))
        assert np.array_equal(A, Ar) and np.array_equal(B, Br), (what, t, int((A != Ar).sum()), int((B != Br).sum()))
        assert rc.same_bits(r, want), (what, t, r, want)
        assert not np.isnan(R).any(), (what, t, "partials not written", np.argwhere(np.isnan(R))[:4])
    if F0 is not None:
        assert np.array_equal(dF.cpu().numpy(), F0)


@pytest.mark.parametrize("cid,ndim,stc,opts", rc.CASES, ids=[c[0] for c in rc.CASES])
def test_residual_cases(torch_cuda, cid, ndim, stc, opts):
    kern = _kernel(opts, stc)
    assert kern.info["residual"] == "max" and kern.residual_elems == 1 + kern.info["grid"] and kern.info["stages"] == 1
    if cid == rc.BIG[0]:
        assert kern.info["stream_blocks"] == 9 and kern.info["tiles_x"] * kern.info["tiles_y"] == 18 and kern.info["grid"] == 168
    spec = oracle.Spec(stc, ndim, rc.step_of(opts))
    A0, B0, F0 = rc.inputs(spec, opts)
    _three_launches(torch_cuda, kern, spec, ndim, opts, A0, B0, F0, cid)


def test_residual_sampled_fuzz(torch_cuda):
    """The seeded sample of the tuner's space: every member that build() compiled, three launches each; at least three quarters of the
    sample are checked (the refusals were decided by the generator and the compiler)."""
    import drstencil_amd as drs
    checked = 0
    for n, (ndim, path, dtype, args, step) in enumerate(rc.sample_jobs()):
        try:
            kern = drs.Kernel(args)
        except drs.KernelBuildError:
            continue
        spec = oracle.Spec(path, ndim, step)
        A0, B0, F0 = rc.inputs(spec, args[:-1])
        _three_launches(torch_cuda, kern, spec, ndim, args[:-1], A0, B0, F0, "sample %02d" % n)
        checked += 1
    assert checked >= rc.MIN_CHECKED, checked


@pytest.mark.parametrize("cid,ndim,stc,opts", rc.PLANT, ids=[c[0] for c in rc.PLANT])
def test_planted_maximum(torch_cuda, cid, ndim, stc, opts):
    """in[p] = 1e3 at one interior cell per launch: corners and both sides of every kind of seam; the other cells' terms are the same in
    every launch, so the reference is the planted cell's neighbourhood against the base launch's maximum -- computed whole on the host once
    per cell all the same (these grids are small)."""
    torch = torch_cuda
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0 = rc.inputs(spec, opts)
    cells = rc.planted_cells(kern.info)
    assert len(cells) >= (14 if cid == rc.BIG[0] else 10), (cid, len(cells))
    dA, dB, dF = _dev(torch, A0, B0, F0)
    for cell in cells:
        dA.copy_(torch.from_numpy(A0))
        dA[cell] = 1e3
        A = A0.copy()
        A[cell] = 1e3
        Br = B0.copy()
        r, R = _launch(torch, kern, dA, dB, dF, A0.dtype)
        want = rc.host_launch(spec, ndim, opts, A, Br, F0)
        print(cid, cell, repr(r), repr(want))
        assert 600 < want < 800 and rc.same_bits(r, want), (cid, cell, r, want)
    assert np.array_equal(dB.cpu().numpy(), Br)


_POISON = rc.PLANT + [rc.EDGE[5], rc.KNOBS[5], rc.MODES[2]]


@pytest.mark.parametrize("cid,ndim,stc,opts", _POISON, ids=[c[0] for c in _POISON])
def test_poison(torch_cuda, cid, ndim, stc, opts):
    """NaN in every cell of `in` that neither a tap nor the centre stream reads, in out's ring, in src's ring and in all of d_res before
    every launch: r is finite and exact, every element of d_res has been overwritten."""
    from footprint import nan_value, ring_mask
    torch = torch_cuda
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0 = rc.inputs(spec, opts)
    ring = ring_mask(spec.shape, spec.halo)
    A = rc.poisoned_input(A0, spec)
    B = B0.copy()
    B[ring] = nan_value(B.dtype)
    if F0 is not None:
        F0[ring] = nan_value(F0.dtype)
    dA, dB, dF = _dev(torch, A, B, F0)
    Ar, Br = A.copy(), B.copy()
    for t in range(2):
        r, R = _launch(torch, kern, dA, dB, dF, A.dtype)
        want = rc.host_launch(spec, ndim, opts, Ar, Br, F0)
        assert np.isfinite(want) and rc.same_bits(r, want), (cid, t, r, want)
        assert not np.isnan(R).any(), (cid, t, np.argwhere(np.isnan(R))[:4])
        Bg = dB.cpu().numpy()
        assert np.array_equal(rc.interior(Bg, spec.halo), rc.interior(Br, spec.halo)) and np.isnan(Bg[ring]).all()


def test_special_values(torch_cuda):
    torch = torch_cuda
    cid, ndim, stc, opts = rc.BIG
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    A0, B0, F0 = rc.inputs(spec, opts)
    mid = tuple(n // 2 for n in spec.shape)

    def one(A):
        dA, dB = _dev(torch, A, B0)
        Ar, Br = A.copy(), B0.copy()
        r, R = _launch(torch, kern, dA, dB, None, A.dtype)
        want = rc.host_launch(spec, ndim, opts, Ar, Br, None)
        assert rc.same_bits(r, want), (r, want)
        assert np.array_equal(np.isnan(dB.cpu().numpy()), np.isnan(Br))
        return r

    A = A0.copy()
    A[mid] = np.nan
    assert np.isnan(one(A))                               # one NaN in an interior cell of in
    assert np.isfinite(one(A0.copy()))                    # ... and no state survives it
    A = A0.copy()
    A[mid] = np.inf                                       # inf - inf at the cell itself
    one(A)
    A[mid[:-1] + (mid[-1] + 3,)] = -np.inf
    one(A)
    Z = np.zeros_like(A0)
    assert one(Z.copy()).tobytes() == np.zeros((), A0.dtype).tobytes()      # +0.0 in bits
    Z[tuple(slice(H, n - H) for n in Z.shape)] = -0.0
    assert one(Z).tobytes() == np.zeros((), A0.dtype).tobytes()


@pytest.mark.parametrize("cid,ndim,stc,opts", rc.UNCHANGED, ids=[c[0] for c in rc.UNCHANGED])
def test_arrays_equal_those_without_the_option(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    torch = torch_cuda
    kern = _kernel(opts, stc)
    plain = drs.Kernel(list(opts) + [stc])
    assert plain.residual_elems == 0 and "residual" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0 = rc.inputs(spec, opts)
    dA1, dB1, dF = _dev(torch, A0, B0, F0)
    dA2, dB2 = _dev(torch, A0, B0)
    src = {"d_src": dF.data_ptr()} if dF is not None else {}
    for t in range(2):
        a, b = ((dA1, dB1), (dB1, dA1))[t]
        _launch(torch, kern, a, b, dF, A0.dtype)
        a, b = ((dA2, dB2), (dB2, dA2))[t]
        plain.launch(a.data_ptr(), b.data_ptr(), **src)
        torch.cuda.synchronize()
        assert torch.equal(dA1, dA2) and torch.equal(dB1, dB2), (cid, t)


@pytest.mark.parametrize("cid,ndim,stc,opts", rc.ARENA, ids=[c[0] for c in rc.ARENA])
def test_residual_guard_bands(torch_cuda, cid, ndim, stc, opts):
    """in, out and a residual array of exactly residual_elems elements carved out of one arena between NaN-with-payload guard bands: after
    a launch every guard element and all of `in` are bit-unchanged, out's ring too, and every element of d_res has been written.  An
    overrun is detected here, never trapped."""
    from footprint import NAN_BITS, int_view
    torch = torch_cuda
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    dt = rc.dtype_of(opts)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    n = int(np.prod(spec.shape))
    guard = 4096 + 4                                     # elements: every array 16-byte aligned, none more than that
    step = -(-(guard + n) // 4) * 4
    off = [guard, guard + step, guard + 2 * step]        # in, out, res
    total = off[2] + kern.residual_elems + guard
    arena = torch.empty(total, dtype=tdt, device="cuda")
    int_view(torch, arena).fill_(NAN_BITS[np.dtype(dt)])
    before = int_view(torch, arena).clone()
    A0, B0, _ = rc.inputs(spec, opts)
    dA = arena[off[0]:off[0] + n].view(spec.shape)
    dB = arena[off[1]:off[1] + n].view(spec.shape)
    dR = arena[off[2]:off[2] + kern.residual_elems]
    dA.copy_(torch.from_numpy(A0))
    inner = tuple(slice(H, s - H) for s in spec.shape)
    dB[inner] = torch.from_numpy(np.ascontiguousarray(B0[inner])).cuda()
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_res=dR.data_ptr())
    torch.cuda.synchronize()
    after = int_view(torch, arena)
    keep = torch.ones(total, dtype=torch.bool, device="cuda")
    keep[off[0]:off[0] + n] = False
    keep[off[1]:off[1] + n] = False
    keep[off[2]:off[2] + kern.residual_elems] = False
    assert torch.equal(after[keep], before[keep]), (cid, "a guard band was written")
    assert np.array_equal(dA.cpu().numpy(), A0), cid
    Br = B0.copy()
    want = rc.host_launch(spec, ndim, opts, A0.copy(), Br, None)
    Bg = dB.cpu().numpy()
    ring = np.ones(spec.shape, bool)
    ring[inner] = False
    assert np.isnan(Bg[ring]).all() and np.array_equal(Bg[inner], Br[inner]), cid
    R = dR.cpu().numpy()
    assert not np.isnan(R).any() and rc.same_bits(R[0], want), (cid, R[0], want)


# ---- run to tolerance ---------------------------------------------------------------------------------------------------------------
def _solve_inputs(spec, dt, F_too):
    H = spec.halo
    shape_i = tuple(n - 2 * H for n in spec.shape)
    A = np.zeros(spec.shape, dt)
    rc.interior(A, H)[...] = np.random.default_rng(21).random(shape_i).astype(dt)      # zero ring, random interior in [0, 1)
    F = None
    if F_too:
        F = np.zeros(spec.shape, dt)
        rc.interior(F, H)[...] = np.random.default_rng(22).random(shape_i).astype(dt) * 0.01
    return A, A.copy(), F


_SOLVE = rc.SOLVE + [rc.POISSON2]


@pytest.mark.parametrize("cid,ndim,stc,opts,tol", _SOLVE, ids=[c[0] for c in _SOLVE])
def test_run_to_tolerance(torch_cuda, cid, ndim, stc, opts, tol):
    """jacobi3 on 18^3 (no centre tap: the centre stream is the only reader of those cells) and the 2D Poisson case: Kernel.solve returns
    status 0 with the launch count, the residual bits and the A of a numpy loop of oracle sweeps that looks at r at the same launches."""
    torch = torch_cuda
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    dt = rc.dtype_of(opts)
    A, B, F = _solve_inputs(spec, dt, "--source" in opts)
    Ar, Br = A.copy(), B.copy()
    want = rc.oracle_solve(spec, Ar, Br, F, tol, rc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and want[1] < rc.MAX_LAUNCHES // 2 and want[1] % 8 == 0, want
    dA, dB, dF = _dev(torch, A, B, F)
    dR = _nan_res(torch, kern, dt)
    status, launches, r = kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), tol, rc.MAX_LAUNCHES, check_every=4, d_src=_ptr(dF))
    print(cid, "launches", launches, "residual", repr(r), "reference", want)
    assert status == 0 and launches == want[1], (status, launches, want)
    assert rc.same_bits(np.asarray(r, dt), want[2]) and kern.residual(dR.data_ptr()) == r
    assert np.array_equal(dA.cpu().numpy(), Ar)
    # max_launches = 16: status 1 with 16 launches
    dA, dB = _dev(torch, A, B)
    assert kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), tol, 16, check_every=4, d_src=_ptr(dF))[:2] == (1, 16)
    # run(): the reference's loop, the last launch's residual
    dA, dB = _dev(torch, A, B)
    n = kern.run(dA.data_ptr(), dB.data_ptr(), iterations=8, **({"d_src": dF.data_ptr()} if dF is not None else {}), d_res=dR.data_ptr())
    Ar, Br = A.copy(), B.copy()
    ref = rc.oracle_solve(spec, Ar, Br, F, 0.0, 8, 4)
    assert n == 8 and rc.same_bits(np.asarray(kern.residual(dR.data_ptr()), dt), ref[2]) and np.array_equal(dA.cpu().numpy(), Ar)


def test_overflow_is_reported(torch_cuda):
    """A centre cell of finfo.max under t3_star's coefficient sum of 1.5: status -4 within a few checks, instead of iterating on inf."""
    torch = torch_cuda
    cid, ndim, stc, opts = rc.DIVERGE
    kern = _kernel(opts, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A = np.ones(spec.shape, np.float32)
    A[tuple(n // 2 for n in spec.shape)] = np.finfo(np.float32).max
    dA, dB = _dev(torch, A, A)
    dR = _nan_res(torch, kern, np.float32)
    status, launches, r = kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), 1e-4, rc.MAX_LAUNCHES, check_every=8)
    print("overflow reported after", launches, "launches:", r)
    assert status == -4 and launches <= 10 * 16 and not np.isfinite(r), (status, launches, r)


def test_emitted_check_program(torch_cuda):
    """The prebuilt --check --residual program: prints the residual line, agrees with gold's arrays, exits 0."""
    exe = rc.check_program_path()
    assert os.path.exists(exe), "build() makes it"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, (p.returncode, out[-1500:], p.stderr[-500:])
    assert "residual : " in out and "[Test] RMS Error: 0.000000e+00" in out and "[Test] Residual Error: 0.000000e+00" in out and "differ" not in out, out[-1500:]
