"""--scale on the MI355X through the C ABI: the case list of tests/scale_cases.py (the one tests/test_scale_cpu.py runs under the
emulation) -- three launches each of dr_ and of gold_, whole arrays bit for bit against the host reference --, unit scale against the same
command without the option, the frozen field, planted factors and their complement, the contracted variants the kernel must not compute,
IEEE special values in w, a guard-band arena, the samples of the tuner's space, the run to tolerance on screened Poisson
(drs_kernel_solve_ops), the operand block on every kind of kernel, a C host and the emitted --check program.
Every kernel is prebuilt by __graft_entry__.build(): nothing here starts hipcc.  The references are computed on the host once per test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import residual_cases as rc
import scale_cases as sc
from footprint import bit_equal, ring_mask
from special_values import count_different, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


def _kernel(full, stc):
    import drstencil_amd as drs
    return drs.Kernel(list(full) + [stc])


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(a).cuda() for a in arrays]


def _kw(dF, dR, dX, dW):
    kw = {"d_scale": dW.data_ptr()}
    if dF is not None:
        kw["d_src"] = dF.data_ptr()
    if dR is not None:
        kw["d_res"] = dR.data_ptr()
    if dX is not None:
        kw["d_fix"] = dX.data_ptr()
    return kw


def _nan_res(torch, kern, dt):
    if not kern.residual_elems:
        return None
    return torch.full((kern.residual_elems,), float("nan"), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")


def _bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def _launches(torch, kern, spec, ndim, opts, A0, B0, F0, X, W, what, launches=3, gold=False):
    """`launches` launches from (A0, B0) with src F0, held cells X and factors W: after each, both WHOLE arrays equal the host reference's
    in bits; with --residual max r equals numpy's in bits and every element of the NaN-filled residual array has been overwritten.
    Afterwards w, src and fix are bit-unchanged."""
    dt = A0.dtype
    dA, dB, dF, dX, dW = _dev(torch, A0, B0, F0, X, W)
    Ar, Br = A0.copy(), B0.copy()
    for t in range(launches):
        s, d = (dA, dB) if t % 2 == 0 else (dB, dA)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        dR = None if gold else _nan_res(torch, kern, dt)
        if gold:
            kern.launch_gold(s.data_ptr(), d.data_ptr(), **_kw(dF, None, dX, dW))
        else:
            kern.launch(s.data_ptr(), d.data_ptr(), **_kw(dF, dR, dX, dW))
        torch.cuda.synchronize()
        want = sc.host_launch(spec, ndim, opts, sr, dr, F0, X, W)
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        assert same_bits(A, Ar) and same_bits(B, Br), (what, t, count_different(A, Ar), count_different(B, Br))
        if dR is not None:
            R = dR.cpu().numpy()
            print(what, "launch", t, "r", repr(R[0]), "reference", repr(want))
            assert rc.same_bits(R[0], want), (what, t, R[0], want)
            assert not np.isnan(R).any() or np.isnan(want), (what, t, "partials not written")
    for d, a in ((dF, F0), (dX, X), (dW, W)):
        assert a is None or bit_equal(d.cpu().numpy(), a), (what, "src, fix or w was written")
    return dA.cpu().numpy(), dB.cpu().numpy()


# ---- 1. bit-exactness -----------------------------------------------------------------------------------------------------------------
_EXACT = sc.CASES + sc.MODES + sc.FORMS


@pytest.mark.parametrize("cid,ndim,stc,opts,c", _EXACT, ids=[c[0] for c in _EXACT])
def test_scale_cases(torch_cuda, cid, ndim, stc, opts, c):
    full = sc.with_scale(opts, c)
    kern = _kernel(full, stc)
    assert kern.scale and kern.scale_centre == c and kern.info["scale"] == 1 and kern.info["stages"] == 1
    assert kern.resources.get("scratch_bytes_per_lane", 0) == 0 and kern.resources.get("sgpr_spill", 0) == 0
    if cid.startswith(sc.BIG[0] + "_c"):
        assert kern.info["stream_blocks"] == 9 and kern.info["tiles_x"] * kern.info["tiles_y"] == 18 and kern.info["grid"] == 168
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W = sc.inputs(spec, full)
    _launches(torch_cuda, kern, spec, ndim, full, A0, B0, F0, X, W, cid)
    _launches(torch_cuda, kern, spec, ndim, full, A0, B0, F0, X, W, (cid, "gold"), gold=True)


# ---- 2. unit scale changes nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", sc.UNCHANGED, ids=[c[0] for c in sc.UNCHANGED])
def test_unit_scale_equals_the_plain_command(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    torch = torch_cuda
    kern = _kernel(sc.with_scale(opts), stc)
    plain = drs.Kernel(list(opts) + [stc])
    assert not plain.scale and "scale" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W = sc.inputs(spec, opts)
    W[...] = 1.0
    dA1, dB1, dF, dW = _dev(torch, A0, B0, F0, W)
    dA2, dB2 = _dev(torch, A0, B0)
    src = {"d_src": dF.data_ptr()} if dF is not None else {}
    for t in range(2):
        a, b = ((dA1, dB1), (dB1, dA1))[t]
        kern.launch(a.data_ptr(), b.data_ptr(), **_kw(dF, None, None, dW))
        a, b = ((dA2, dB2), (dB2, dA2))[t]
        plain.launch(a.data_ptr(), b.data_ptr(), **src)
        torch.cuda.synchronize()
        assert bit_equal(dA1.cpu().numpy(), dA2.cpu().numpy()) and bit_equal(dB1.cpu().numpy(), dB2.cpu().numpy()), (cid, t)


# ---- 3. frozen field ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", sc.FROZEN, ids=[c[0] for c in sc.FROZEN])
def test_frozen_field(torch_cuda, cid, ndim, stc, opts):
    """w = 0 and centre 1 on inputs without zeros or non-finite values: out equals in on the interior, in bits, and out's ring is untouched."""
    torch = torch_cuda
    full = sc.with_scale(opts, 1)
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W = sc.inputs(spec, full)
    assert np.isfinite(A0).all() and (A0 != 0).all()
    W[...] = 0.0
    Ar, Br = A0.copy(), B0.copy()
    sc.host_launch(spec, ndim, full, Ar, Br, None, None, W)
    want = B0.copy()
    rc.interior(want, spec.halo)[...] = rc.interior(A0, spec.halo)
    assert bit_equal(Br, want) and bit_equal(Ar, A0)                       # on the reference alone
    for gold in (False, True):
        dA, dB, dW = _dev(torch, A0, B0, W)
        (kern.launch_gold if gold else kern.launch)(dA.data_ptr(), dB.data_ptr(), d_scale=dW.data_ptr())
        torch.cuda.synchronize()
        assert bit_equal(dB.cpu().numpy(), want) and bit_equal(dA.cpu().numpy(), A0), (cid, gold)


# ---- 4. planted factors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", sc.PLANT, ids=[c[0] for c in sc.PLANT])
def test_planted_factors(torch_cuda, cid, ndim, stc, opts):
    """w = 1 except at the interior corners and both sides of every x, y and z seam, each with a factor 2 + n/64 of its own; then the
    complement.  Every cell equals the reference in bits, and the cells that differ from the unit-scale run are exactly the planted ones."""
    full = sc.with_scale(opts)
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, _ = sc.inputs(spec, full)
    cells = rc.planted_cells(kern.info)
    assert len(cells) >= (14 if cid.startswith(sc.BIG[0]) else 10), (cid, len(cells))
    planted = np.zeros(spec.shape, bool)
    vals = np.ones(spec.shape, A0.dtype)
    for n, c in enumerate(cells):
        planted[c] = True
        vals[c] = 2 + n / 64
    inner = ~ring_mask(spec.shape, spec.halo)
    unit = B0.copy()
    sc.host_launch(spec, ndim, full, A0.copy(), unit, None, None, np.ones(spec.shape, A0.dtype))
    every = (2 + (np.arange(planted.size).reshape(planted.shape) % 64) / 64).astype(A0.dtype)
    for mask, W in ((planted, vals), (~planted & inner, np.where(~planted & inner, every, 1).astype(A0.dtype))):
        Br = B0.copy()
        sc.host_launch(spec, ndim, full, A0.copy(), Br, None, None, W)
        assert np.array_equal(_bits(Br) != _bits(unit), mask), (cid, int(mask.sum()))                    # on the reference alone
        A, B = _launches(torch_cuda, kern, spec, ndim, full, A0, B0, None, None, W, (cid, int(mask.sum())), launches=1)
        assert np.array_equal(_bits(B) != _bits(unit), mask), (cid, int(mask.sum()))
        _launches(torch_cuda, kern, spec, ndim, full, A0, B0, None, None, W, (cid, int(mask.sum()), "gold"), launches=1, gold=True)


# ---- 5. no contraction ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", sc.CONTRACTION, ids=[c[0] for c in sc.CONTRACTION])
def test_no_contraction(torch_cuda, cid, ndim, stc, opts):
    """Centre 0.3: a kernel that contracted w * v + t or C * in + (w * v) into an FMA would differ from the contract in at least one cell
    (asserted on the reference alone: fp32 through exact float64 products, fp64 in rationals on a few hundred cells); the kernel equals
    the contract in bits."""
    full = sc.with_scale(opts, 0.3)
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W = sc.inputs(spec, full)
    cells = None
    if A0.dtype == np.float64:
        cells = np.zeros(rc.interior(A0, spec.halo).shape, bool)
        cells.reshape(-1)[np.random.default_rng(3).choice(cells.size, 300, replace=False)] = True
    Br = B0.copy()
    sc.host_launch(spec, ndim, full, A0.copy(), Br, None, None, W)
    for variant in ("fma_w", "fma_c"):
        Bv = Br.copy()                                                    # outside `cells` the contract's values stand
        sc.host_launch(spec, ndim, full, A0.copy(), Bv, None, None, W, variant=variant, cells=cells)
        nd = count_different(Bv, Br)
        print(cid, variant, "cells that a contraction would change:", nd)
        assert nd >= 1, (cid, variant, "the contracted variant equals the contract on this seed")
    A, B = _launches(torch_cuda, kern, spec, ndim, full, A0, B0, None, None, W, cid, launches=1)
    assert bit_equal(B, Br)
    _launches(torch_cuda, kern, spec, ndim, full, A0, B0, None, None, W, (cid, "gold"), launches=1, gold=True)


# ---- 6. special values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("held", [False, True], ids=["free", "dirichlet"])
@pytest.mark.parametrize("cid,ndim,stc,opts", sc.SPECIAL, ids=[c[0] for c in sc.SPECIAL])
def test_special_values(torch_cuda, cid, ndim, stc, opts, held):
    """w holds +0.0, -0.0, +-inf, NaN and the smallest subnormals at corners and seams; `in` is planted so that S(in) is inf where w = 0
    (-> NaN), -0.0 where w = -0.0 and finite where w = inf.  NaN where the reference is NaN, bits elsewhere; with --dirichlet a held cell
    whose scaled value is NaN still stores fix[p]."""
    full = sc.with_scale(list(opts) + (sc.DIR if held else []), 1)
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W, cells = sc.special_problem(spec, full, kern.info)
    S = B0.copy()
    oracle.sweep(spec, A0.copy(), S, contract=1)
    Br = B0.copy()
    sc.host_launch(spec, ndim, full, A0.copy(), Br, None, X, W)
    p, q, s = cells["zero_times_inf"], cells["inf_times_fin"], cells["m0_times_m0"]
    m0 = np.asarray(-0.0, A0.dtype).tobytes()
    assert np.isinf(S[p]) and W[p] == 0 and (Br[p] == 0.5 if held else np.isnan(Br[p]))                  # on the reference alone
    assert np.isfinite(S[q]) and S[q] != 0 and np.isinf(W[q]) and np.isinf(Br[q])
    assert S[s].tobytes() == m0 and W[s].tobytes() == m0
    for gold in (False, True):
        _launches(torch_cuda, kern, spec, ndim, full, A0, B0, None, X, W, (cid, held, gold), launches=2, gold=gold)


# ---- 7. memory contract: a guard-band arena -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", sc.ARENA, ids=[c[0] for c in sc.ARENA])
def test_scale_guard_bands(torch_cuda, cid, ndim, stc, opts):
    """in, out and w carved out of one arena between NaN-with-payload guard bands; w's ring is NaN.  After a launch every guard element,
    all of `in` and all of w are bit-unchanged, out's ring too.  An overrun is detected here, never trapped."""
    from footprint import NAN_BITS, int_view
    torch = torch_cuda
    full = sc.with_scale(opts, 2)
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    dt = sc.dtype_of(opts)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    n = int(np.prod(spec.shape))
    guard = 4096 + 4                                     # elements: every array 16-byte aligned, none more than that
    step = -(-(guard + n) // 4) * 4
    off = [guard, guard + step, guard + 2 * step]        # in, out, w
    total = off[2] + n + guard
    arena = torch.empty(total, dtype=tdt, device="cuda")
    int_view(torch, arena).fill_(NAN_BITS[np.dtype(dt)])
    before = int_view(torch, arena).clone()
    A0, B0, _, _, W = sc.inputs(spec, full)
    ring = ring_mask(spec.shape, H)
    W[ring] = np.nan
    dA = arena[off[0]:off[0] + n].view(spec.shape)
    dB = arena[off[1]:off[1] + n].view(spec.shape)
    dW = arena[off[2]:off[2] + n].view(spec.shape)
    dA.copy_(torch.from_numpy(A0))
    dW.copy_(torch.from_numpy(W))
    inner = tuple(slice(H, s - H) for s in spec.shape)
    dB[inner] = torch.from_numpy(np.ascontiguousarray(B0[inner])).cuda()
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_scale=dW.data_ptr())
    torch.cuda.synchronize()
    after = int_view(torch, arena)
    keep = torch.ones(total, dtype=torch.bool, device="cuda")
    for o in off:
        keep[o:o + n] = False
    assert torch.equal(after[keep], before[keep]), (cid, "a guard band was written")
    assert bit_equal(dA.cpu().numpy(), A0) and bit_equal(dW.cpu().numpy(), W), cid
    Br = B0.copy()
    sc.host_launch(spec, ndim, full, A0.copy(), Br, None, None, W)
    Bg = dB.cpu().numpy()
    assert not np.isnan(Br[inner]).any()
    assert np.isnan(Bg[ring]).all() and bit_equal(np.ascontiguousarray(Bg[inner]), np.ascontiguousarray(Br[inner])), cid


# ---- 8. the samples of the tuner's space ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(sc.SAMPLES))
def test_scale_sampled_fuzz(torch_cuda, which):
    """A seeded sample of the tuner's space: every member that build() compiled, three launches each; the refused ones are those the case
    file lists (decided by the generator and the compiler), at most 5 of 20."""
    import drstencil_amd as drs
    checked, refused = 0, []
    for n, (ndim, path, dtype, args, step) in enumerate(sc.sample_jobs(which)):
        try:
            kern = drs.Kernel(args)
        except drs.KernelBuildError:
            refused.append(n)
            continue
        spec = oracle.Spec(path, ndim, step)
        A0, B0, F0, X, W = sc.inputs(spec, args[:-1])
        _launches(torch_cuda, kern, spec, ndim, args[:-1], A0, B0, F0, X, W, "%s %02d" % (which, n))
        checked += 1
    assert checked >= sc.MIN_CHECKED and refused == [n for n, _ in sc.REFUSED[which]], (checked, refused)


# ---- 9. run to tolerance --------------------------------------------------------------------------------------------------------------
_SOLVE = [(c[0] + ("_held" if h else ""), c[1], c[2], c[3], c[4], h) for c in sc.SOLVE for h in (False, True)]


@pytest.mark.parametrize("cid,ndim,stc,opts,tol,held", _SOLVE, ids=[c[0] for c in _SOLVE])
def test_run_to_tolerance(torch_cuda, cid, ndim, stc, opts, tol, held):
    """Screened Poisson on 18^3 as the Jacobi sweep u' = w * S(u) + src: Kernel.solve (drs_kernel_solve_ops) returns the status, the launch
    count and the r of a numpy loop of the host reference that looks at r at the same launches; both arrays and w equal it in bits; once
    more with an inner block held through d_fix.  Fewer launches than the same problem with sigma = 0 (asserted on the reference alone)."""
    torch = torch_cuda
    kern = _kernel(sc.solve_opts(opts, held), stc)
    spec = oracle.Spec(stc, ndim, 1)
    dt = sc.dtype_of(opts)
    A, B, F, X, W = sc.solve_problem(spec, dt, held=held)
    Ar, Br = A.copy(), B.copy()
    want = sc.oracle_solve(spec, Ar, Br, F, X, W, tol, sc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and want[1] < sc.MAX_LAUNCHES and want[1] % 8 == 0, want
    A1, B1, F1, X1, W1 = sc.solve_problem(spec, dt, sigma=False, held=held)
    unscreened = sc.oracle_solve(spec, A1, B1, F1, X1, W1, tol, sc.MAX_LAUNCHES, 4)
    assert unscreened[0] == 0 and want[1] < unscreened[1], (want, unscreened)
    dA, dB, dF, dX, dW = _dev(torch, A, B, F, X, W)
    dR = _nan_res(torch, kern, dt)
    kw = _kw(dF, None, dX, dW)
    status, launches, r = kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), tol, sc.MAX_LAUNCHES, check_every=4, **kw)
    print(cid, "launches", launches, "residual", repr(r), "reference", want, "sigma = 0:", unscreened[1])
    assert status == 0 and launches == want[1], (status, launches, want)
    assert rc.same_bits(np.asarray(r, dt), want[2]) and kern.residual(dR.data_ptr()) == r
    Ag, Bg = dA.cpu().numpy(), dB.cpu().numpy()
    assert bit_equal(Ag, Ar) and bit_equal(Bg, Br) and bit_equal(dW.cpu().numpy(), W)
    if held:
        h = ~np.isnan(X)
        assert bit_equal(Ag[h], X[h]) and bit_equal(Bg[h], X[h])
    # max_launches = 16: status 1 with 16 launches; run() and run_timed(): the reference's loop
    dA, dB = _dev(torch, A, B)
    assert kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), tol, 16, check_every=4, **kw)[:2] == (1, 16)
    dA, dB = _dev(torch, A, B)
    n = kern.run(dA.data_ptr(), dB.data_ptr(), iterations=8, d_res=dR.data_ptr(), **kw)
    Ar, Br = A.copy(), B.copy()
    ref = sc.oracle_solve(spec, Ar, Br, F, X, W, 0.0, 8, 4)
    assert n == 8 and rc.same_bits(np.asarray(kern.residual(dR.data_ptr()), dt), ref[2]) and bit_equal(dA.cpu().numpy(), Ar)
    n, ms = kern.run_timed(dA.data_ptr(), dB.data_ptr(), iterations=4, warmup=0, d_res=dR.data_ptr(), **kw)
    assert n == 4 and ms > 0
    sc.oracle_solve(spec, Ar, Br, F, X, W, 0.0, 4, 2)
    assert bit_equal(dA.cpu().numpy(), Ar)
    # the gold loop through the operand block: no residual
    dA, dB = _dev(torch, A, B)
    assert kern.run(dA.data_ptr(), dB.data_ptr(), iterations=8, gold=True, **kw) == 8
    Ar, Br = A.copy(), B.copy()
    sc.oracle_solve(spec, Ar, Br, F, X, W, 0.0, 8, 4)
    torch.cuda.synchronize()
    assert bit_equal(dA.cpu().numpy(), Ar)


# ---- 10. the operand block on every kind of kernel, the C host, the emitted program ---------------------------------------------------
def test_operand_block_runs_old_kinds(torch_cuda):
    """drs_kernel_launch_ops / _launch_gold_ops / _run_ops on a plain, a --source, a --dirichlet and a --residual max kernel: the arrays of
    the kernel's own family of entry points, in bits."""
    import dirichlet_cases as dc
    import drstencil_amd as drs
    torch = torch_cuda
    L = drs.lib()
    cid, ndim, stc, opts = sc.EDGE[1]
    spec = oracle.Spec(stc, ndim, 1)
    for extra in ([], sc.SOURCE, sc.DIR, rc.RES):
        full = list(opts) + extra
        kern = drs.Kernel(full + [stc])
        A0, B0, F0 = rc.inputs(spec, full)
        X = dc.fix_pattern(spec.shape, A0.dtype) if extra == sc.DIR else None
        dA, dB, dF, dX = _dev(torch, A0, B0, F0, X)
        dR = _nan_res(torch, kern, A0.dtype)
        ptr = lambda d: None if d is None else d.data_ptr()          # noqa: E731
        ops = ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands), ptr(dF), ptr(dR), ptr(dX), None))
        gops = ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands), ptr(dF), None, ptr(dX), None))
        assert L.drs_kernel_launch_ops(kern.h, dA.data_ptr(), dB.data_ptr(), ops, 0) == 0
        assert L.drs_kernel_run_ops(kern.h, dB.data_ptr(), dA.data_ptr(), ops, 2, 0, 0) == 2
        torch.cuda.synchronize()
        kw = {k: v.data_ptr() for k, v in (("d_src", dF), ("d_fix", dX)) if v is not None}
        eA, eB = _dev(torch, A0, B0)
        eR = _nan_res(torch, kern, A0.dtype)
        rkw = dict(kw, **({"d_res": eR.data_ptr()} if eR is not None else {}))
        kern.launch(eA.data_ptr(), eB.data_ptr(), **rkw)
        assert kern.run(eB.data_ptr(), eA.data_ptr(), iterations=2, **rkw) == 2
        torch.cuda.synchronize()
        assert bit_equal(dA.cpu().numpy(), eA.cpu().numpy()) and bit_equal(dB.cpu().numpy(), eB.cpu().numpy()), extra
        if dR is not None:
            assert bit_equal(dR.cpu().numpy(), eR.cpu().numpy())
        gA, gB = _dev(torch, A0, B0)
        assert L.drs_kernel_launch_gold_ops(kern.h, gA.data_ptr(), gB.data_ptr(), gops, 0) == 0
        assert L.drs_kernel_run_ops(kern.h, gB.data_ptr(), gA.data_ptr(), gops, 2, 1, 0) == 2
        torch.cuda.synchronize()
        assert bit_equal(gA.cpu().numpy(), eA.cpu().numpy()) and bit_equal(gB.cpu().numpy(), eB.cpu().numpy()), (extra, "gold")
        ms = ctypes.c_float()
        assert L.drs_kernel_run_timed_ops(kern.h, dA.data_ptr(), dB.data_ptr(), ops, 2, 1, 0, ctypes.byref(ms)) == 2 and ms.value > 0


def test_c_host_through_the_operand_block(torch_cuda):
    """tests/native/capi_ops_host.c, built by build(): a heterogeneous heat step on tests/stc/lap3.stc through drs_kernel_run_ops, the gold
    kernel with the same operands, and the refusals."""
    exe = sc.c_host_path()
    assert os.path.exists(exe), "build() makes it"
    spec = oracle.Spec(sc.LAP3, 3, 1)
    L, M, N = spec.shape
    p = subprocess.run([exe, sc.LAP3, str(L), str(M), str(N), str(spec.halo)], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, (p.returncode, out[-1500:], p.stderr[-500:])
    # bit-identical to the gold kernel: max_abs is the metric's floor of 1e-13, as in test_c_host_through_the_abi
    assert "launches 4 gold_launches 4 one 0 gold_one 0 ms_positive 1 rms 0.000e+00 max_abs 1.000e-13 max_rel 0.000e+00" in out, out
    assert "refusals old -2 missing -2 superfluous -2 size -2 solve -2" in out, out


def test_emitted_check_program(torch_cuda):
    """The prebuilt --check --scale program (periodic, order 2, source, scale, centre 2): dr_ and gold_ run with the same w and agree."""
    exe = sc.check_program_path()
    assert os.path.exists(exe), "build() makes it"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, (p.returncode, out[-1500:], p.stderr[-500:])
    assert "[Test] RMS Error: 0.000000e+00" in out and "differ" not in out, out[-1500:]
