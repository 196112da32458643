"""--varcoef on the MI355X through the C ABI: the case list of tests/varcoef_cases.py (the one tests/test_varcoef_cpu.py runs under the
emulation) -- three launches each of dr_ and of gold_, whole arrays bit for bit against the host reference (the gold-order chain with
libm's correctly rounded fma) --, constant arrays against the same command without the option and against the oracle, exact small
integers (once at 448^3 fp64, where the last tap's grid starts past byte offset 2^32), tap identity, IEEE special values in the
coefficients, a guard-band arena, the sample of the tuner's space, the run to tolerance on -div(kappa grad u) = f
(drs_kernel_solve_ops), the operand block with coef set on old kinds of kernel, and the emitted --check program.
Every kernel is prebuilt by __graft_entry__.build(): nothing here starts a compiler.  The references are computed on the host once per test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import residual_cases as rc
import scale_cases as sc
import varcoef_cases as vc
from footprint import bit_equal, ring_mask
from special_values import count_different, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(vc.fma_lib_path()), "build() makes the reference's fma"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


def _kernel(full, stc):
    import drstencil_amd as drs
    return drs.Kernel(list(full) + [stc])


def _dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(a).cuda() for a in arrays]


def _kw(dF, dR, dX, dW, dK):
    kw = {"d_coef": dK.data_ptr()}
    for name, d in (("d_src", dF), ("d_res", dR), ("d_fix", dX), ("d_scale", dW)):
        if d is not None:
            kw[name] = d.data_ptr()
    return kw


def _nan_res(torch, kern, dt):
    if not kern.residual_elems:
        return None
    return torch.full((kern.residual_elems,), float("nan"), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")


def _launches(torch, kern, spec, ndim, opts, A0, B0, F0, X, W, K, what, launches=3, gold=False):
    """`launches` launches from (A0, B0): after each, both WHOLE arrays equal the host reference's in bits; with --residual max r equals
    numpy's in bits and every element of the NaN-filled residual array has been overwritten.  Afterwards coef, w, src and fix are
    bit-unchanged."""
    dt = A0.dtype
    dA, dB, dF, dX, dW, dK = _dev(torch, A0, B0, F0, X, W, K)
    Ar, Br = A0.copy(), B0.copy()
    for t in range(launches):
        s, d = (dA, dB) if t % 2 == 0 else (dB, dA)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        dR = None if gold else _nan_res(torch, kern, dt)
        if gold:
            kern.launch_gold(s.data_ptr(), d.data_ptr(), **_kw(dF, None, dX, dW, dK))
        else:
            kern.launch(s.data_ptr(), d.data_ptr(), **_kw(dF, dR, dX, dW, dK))
        torch.cuda.synchronize()
        want = vc.host_launch(spec, ndim, opts, sr, dr, F0, X, W, K)
        A, B = dA.cpu().numpy(), dB.cpu().numpy()
        assert same_bits(A, Ar) and same_bits(B, Br), (what, t, count_different(A, Ar), count_different(B, Br))
        if dR is not None:
            R = dR.cpu().numpy()
            print(what, "launch", t, "r", repr(R[0]), "reference", repr(want))
            assert rc.same_bits(R[0], want), (what, t, R[0], want)
            assert not np.isnan(R).any() or np.isnan(want), (what, t, "partials not written")
    for d, a in ((dF, F0), (dX, X), (dW, W), (dK, K)):
        assert a is None or bit_equal(d.cpu().numpy(), a), (what, "src, fix, w or coef was written")
    return dA.cpu().numpy(), dB.cpu().numpy()


# ---- bit-exactness --------------------------------------------------------------------------------------------------------------------
_EXACT = vc.CASES + vc.MODES


@pytest.mark.parametrize("cid,ndim,stc,opts", _EXACT, ids=[c[0] for c in _EXACT])
def test_varcoef_cases(torch_cuda, cid, ndim, stc, opts):
    full = vc.with_vc(opts)
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    assert kern.varcoef and kern.info["stages"] == 1 and kern.coef_taps == tuple(o for o, _ in spec.points)
    assert kern.resources.get("scratch_bytes_per_lane", 0) == 0 and kern.resources.get("sgpr_spill", 0) == 0
    if cid.startswith(vc.BIG[0]):
        i = kern.info          # 16 x 4 lanes, 9 stream blocks of 54 tiles, and more launched workgroups than tiles: some leave at once
        assert i["threads"] == 64 and i["stream_blocks"] == 9 and i["tiles_x"] * i["tiles_y"] == 54 and i["grid"] == 488 > 486
    A0, B0, F0, X, W, K = vc.inputs(spec, full)
    _launches(torch_cuda, kern, spec, ndim, full, A0, B0, F0, X, W, K, cid)
    _launches(torch_cuda, kern, spec, ndim, full, A0, B0, F0, X, W, K, (cid, "gold"), gold=True)


# ---- constant arrays change nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", vc.UNCHANGED, ids=[c[0] for c in vc.UNCHANGED])
def test_constant_arrays_equal_the_plain_command(torch_cuda, cid, ndim, stc, opts):
    """a_t[p] = (real_t)(c_t) everywhere: the stored bits are those of the same command without the option, and of oracle.sweep(contract=1)."""
    import drstencil_amd as drs
    torch = torch_cuda
    kern = _kernel(vc.with_vc(opts), stc)
    plain = drs.Kernel(list(opts) + [stc])
    assert not plain.varcoef and "varcoef" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W, _ = vc.inputs(spec, opts)
    K = vc.constant_coefficients(spec, A0.dtype)
    dA1, dB1, dK = _dev(torch, A0, B0, K)
    dA2, dB2 = _dev(torch, A0, B0)
    A3, B3 = A0.copy(), B0.copy()
    for t in range(2):
        a, b = ((dA1, dB1), (dB1, dA1))[t]
        kern.launch(a.data_ptr(), b.data_ptr(), d_coef=dK.data_ptr())
        a, b = ((dA2, dB2), (dB2, dA2))[t]
        plain.launch(a.data_ptr(), b.data_ptr())
        torch.cuda.synchronize()
        assert bit_equal(dA1.cpu().numpy(), dA2.cpu().numpy()) and bit_equal(dB1.cpu().numpy(), dB2.cpu().numpy()), (cid, t)
        a, b = ((A3, B3), (B3, A3))[t]
        oracle.sweep(spec, a, b, contract=1)
        assert bit_equal(dA1.cpu().numpy(), A3) and bit_equal(dB1.cpu().numpy(), B3), (cid, t, "oracle")


# ---- exact integers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", vc.INTEGER, ids=[c[0] for c in vc.INTEGER])
def test_exact_integers(torch_cuda, cid, ndim, stc, opts):
    """in in [-4, 4], a_t[p] = ((7 t + hash(p)) mod 7) - 3: every product and sum is exact, and plain integer numpy is the reference."""
    torch = torch_cuda
    kern = _kernel(vc.with_vc(opts), stc)
    spec = oracle.Spec(stc, ndim, 1)
    A, K, want = vc.integer_problem(spec, np.dtype(vc.dtype_of(opts)))
    for gold in (False, True):
        B = np.full(A.shape, 0.5, A.dtype)
        dA, dB, dK = _dev(torch, A, B, K)
        (kern.launch_gold if gold else kern.launch)(dA.data_ptr(), dB.data_ptr(), d_coef=dK.data_ptr())
        torch.cuda.synchronize()
        B = dB.cpu().numpy()
        got = rc.interior(B, spec.halo)
        assert np.array_equal(got, want.astype(A.dtype)), (cid, gold, int((got != want).sum()))
        assert (B[ring_mask(spec.shape, spec.halo)] == 0.5).all()


def test_exact_integers_past_4gib(torch_cuda):
    """3d7pt_star fp64 at 448^3: a grid is 448^3 * 8 = 719 323 136 bytes, so tap 6's grid starts at byte 4 315 938 816 > 2^32 -- the smallest
    cube at which a 32-bit offset of the last grid goes wrong.  Inputs and coefficients are generated on the device with the rule of
    varcoef_cases.integer_problem's kind (small integers from an index hash), the reference is exact integer arithmetic on the device's
    own copy, and three thin slabs (bottom, middle, top) are compared on the host."""
    torch = torch_cuda
    n = vc.INT_BIG_DIM
    stc = vc.int_big_stc()
    kern = _kernel(vc.with_vc(vc.INT_BIG_OPTS), stc)
    spec = oracle.Spec(stc, 3, 1)
    H = spec.halo
    taps = vc.taps_of(spec)
    T = len(taps)
    assert T == 7 and (T - 1) * n ** 3 * 8 > 2 ** 32 and kern.info["N"] == n
    idx = torch.arange(n ** 3, dtype=torch.int64, device="cuda")
    h = ((idx * 2654435761) >> 7) & 0xFFFFFFFF
    dA = ((h % 9) - 4).to(torch.float64).view(n, n, n)
    dK = torch.empty((T, n, n, n), dtype=torch.float64, device="cuda")
    for t in range(T):
        ht = (((idx + t * n ** 3) * 2654435761) >> 7) & 0xFFFFFFFF          # the hash of the element's index in the whole (T, grid) array
        dK[t] = ((7 * t + ht) % 7 - 3).to(torch.float64).view(n, n, n)
    del idx, h, ht
    dB = torch.full((n, n, n), 0.5, dtype=torch.float64, device="cuda")
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_coef=dK.data_ptr())
    torch.cuda.synchronize()
    for z0 in (H, n // 2 - 2, n - H - 4):
        zs = slice(z0, z0 + 4)
        A = dA[z0 - H:z0 + 4 + H].cpu().numpy().astype(np.int64)
        want = np.zeros((4, n - 2 * H, n - 2 * H), np.int64)
        for t, (dz, dy, dx) in enumerate(taps):
            k = dK[t, zs, H:n - H, H:n - H].cpu().numpy().astype(np.int64)
            want += k * A[H + dz:H + dz + 4, H + dy:n - H + dy, H + dx:n - H + dx]
        got = dB[zs, H:n - H, H:n - H].cpu().numpy()
        assert np.abs(want).max() > 8
        assert np.array_equal(got, want.astype(np.float64)), (z0, int((got != want).sum()))
    assert float(dB[0, 0, 0]) == 0.5 and float(dB[n - 1, n - 1, n - 1]) == 0.5


# ---- tap identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", vc.IDENTITY, ids=[c[0] for c in vc.IDENTITY])
def test_tap_identity(torch_cuda, cid, ndim, stc, opts):
    """Coefficients zero everywhere except one tap's grid at one cell, for every tap in turn, at a corner cell, a seam cell and an interior
    cell: exactly that cell differs from zero, by exactly a * in[p + d_t]."""
    torch = torch_cuda
    kern = _kernel(vc.with_vc(opts), stc)
    spec = oracle.Spec(stc, ndim, 1)
    A = vc.inputs(spec, opts)[0]
    taps = vc.taps_of(spec)
    a = np.asarray(1.25, A.dtype)
    dA = torch.from_numpy(A).cuda()
    ring = ring_mask(spec.shape, spec.halo)
    for cell in vc.identity_cells(kern.info, A.shape):
        for t, d in enumerate(taps):
            K = np.zeros((len(taps),) + A.shape, A.dtype)
            K[t][cell] = a
            dB = torch.full(A.shape, 0.5, dtype=dA.dtype, device="cuda")
            dK = torch.from_numpy(K).cuda()
            kern.launch(dA.data_ptr(), dB.data_ptr(), d_coef=dK.data_ptr())
            torch.cuda.synchronize()
            B = dB.cpu().numpy()
            want = np.zeros(A.shape, A.dtype)
            want[ring] = 0.5
            want[cell] = a * A[tuple(c + o for c, o in zip(cell, d))]
            assert want[cell] != 0 and np.array_equal(B, want), (cid, cell, t, np.argwhere(B != want)[:4])


# ---- special values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("held", [False, True], ids=["free", "dirichlet"])
@pytest.mark.parametrize("cid,ndim,stc,opts", vc.SPECIAL, ids=[c[0] for c in vc.SPECIAL])
def test_special_values(torch_cuda, cid, ndim, stc, opts, held):
    """Coefficients holding +0.0, -0.0, +-inf, NaN and the smallest subnormals at corners and seams, +inf and -0.0 planted in `in`: NaN where
    the reference is NaN, bits elsewhere; with --dirichlet a held cell whose sum is not finite still stores fix[p]."""
    full = vc.with_vc(list(opts) + (vc.DIR if held else []))
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W, K, p, q = vc.special_problem(spec, full, kern.info, held)
    Br = B0.copy()
    vc.host_launch(spec, ndim, full, A0.copy(), Br, F0, X, W, K)
    assert (Br[p] == 0.5 if held else not np.isfinite(Br[p])) and Br[q] == 0          # on the reference alone
    for gold in (False, True):
        _launches(torch_cuda, kern, spec, ndim, full, A0, B0, F0, X, W, K, (cid, held, gold), launches=2, gold=gold)


# ---- memory contract: a guard-band arena ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts", vc.ARENA, ids=[c[0] for c in vc.ARENA])
def test_varcoef_guard_bands(torch_cuda, cid, ndim, stc, opts):
    """in, out, src, coef and the residual array carved out of one arena between NaN-with-payload guard bands; the ring of every coefficient
    grid and of src is NaN.  After a launch every guard element, all of `in`, src and coef are bit-unchanged, out's ring too.  An overrun is
    detected here, never trapped."""
    from footprint import NAN_BITS, int_view
    torch = torch_cuda
    full = vc.with_vc(list(opts) + vc.SOURCE + rc.RES)
    kern = _kernel(full, stc)
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    dt = vc.dtype_of(opts)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    A0, B0, F0, _, _, K = vc.inputs(spec, full)
    n, T = int(np.prod(spec.shape)), len(K)
    guard = 4096 + 4                                     # elements: every array 16-byte aligned, none more than that
    sizes = [n, n, n, T * n, -(-kern.residual_elems // 4) * 4]          # in, out, src, coef, res
    off, at = [], guard
    for s in sizes:
        off.append(at)
        at += -(-(s + guard) // 4) * 4
    total = at
    arena = torch.empty(total, dtype=tdt, device="cuda")
    int_view(torch, arena).fill_(NAN_BITS[np.dtype(dt)])
    before = int_view(torch, arena).clone()
    ring = ring_mask(spec.shape, H)
    K[:, ring] = np.nan
    F0[ring] = np.nan
    dA = arena[off[0]:off[0] + n].view(spec.shape)
    dB = arena[off[1]:off[1] + n].view(spec.shape)
    dF = arena[off[2]:off[2] + n].view(spec.shape)
    dK = arena[off[3]:off[3] + T * n].view(K.shape)
    dR = arena[off[4]:off[4] + kern.residual_elems]
    dA.copy_(torch.from_numpy(A0))
    dF.copy_(torch.from_numpy(F0))
    dK.copy_(torch.from_numpy(K))
    inner = tuple(slice(H, s - H) for s in spec.shape)
    dB[inner] = torch.from_numpy(np.ascontiguousarray(B0[inner])).cuda()
    kern.launch(dA.data_ptr(), dB.data_ptr(), d_src=dF.data_ptr(), d_res=dR.data_ptr(), d_coef=dK.data_ptr())
    torch.cuda.synchronize()
    after = int_view(torch, arena)
    keep = torch.ones(total, dtype=torch.bool, device="cuda")
    for o, s in zip(off, sizes[:4] + [kern.residual_elems]):
        keep[o:o + s] = False
    assert torch.equal(after[keep], before[keep]), (cid, "a guard band was written")
    assert bit_equal(dA.cpu().numpy(), A0) and bit_equal(dK.cpu().numpy(), K) and bit_equal(dF.cpu().numpy(), F0), cid
    Br = B0.copy()
    want = vc.host_launch(spec, ndim, full, A0.copy(), Br, F0, None, None, K)
    Bg = dB.cpu().numpy()
    assert not np.isnan(Br[inner]).any()
    assert np.isnan(Bg[ring]).all() and bit_equal(np.ascontiguousarray(Bg[inner]), np.ascontiguousarray(Br[inner])), cid
    assert rc.same_bits(dR.cpu().numpy()[0], want)


# ---- the sample of the tuner's space --------------------------------------------------------------------------------------------------
def test_varcoef_sampled_fuzz(torch_cuda):
    """A seeded sample of the tuner's space: every member that build() compiled, three launches each; the refused ones are those the case
    file lists (decided by the generator and the compiler), at most 5 of 20."""
    import drstencil_amd as drs
    checked, refused = 0, []
    for n, (ndim, path, dtype, args, step) in enumerate(vc.sample_jobs()):
        try:
            kern = drs.Kernel(args)
        except drs.KernelBuildError:
            refused.append(n)
            continue
        spec = oracle.Spec(path, ndim, step)
        A0, B0, F0, X, W, K = vc.inputs(spec, args[:-1])
        _launches(torch_cuda, kern, spec, ndim, args[:-1], A0, B0, F0, X, W, K, "sample %02d" % n)
        checked += 1
    assert checked >= vc.MIN_CHECKED and refused == [n for n, _ in vc.REFUSED], (checked, refused)


# ---- run to tolerance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts,tol", vc.SOLVE, ids=[c[0] for c in vc.SOLVE])
def test_run_to_tolerance(torch_cuda, cid, ndim, src, opts, tol):
    """Jacobi for -div(kappa grad u) = 1 with a two-valued kappa: Kernel.solve (drs_kernel_solve_ops) returns the status, the launch count
    and the r of a numpy loop of the host reference that looks at r at the same launches; both arrays equal it in bits."""
    torch = torch_cuda
    stc = os.path.join(vc.gpu_stc_dir(), "divgrad%d.stc" % ndim)
    assert os.path.exists(stc), "build() writes it"
    kern = _kernel(vc.solve_opts(opts), stc)
    spec = oracle.Spec(stc, ndim, 1)
    dt = vc.dtype_of(opts)
    A, B, F, K = vc.divgrad_problem(spec, dt)
    Ar, Br = A.copy(), B.copy()
    want = vc.oracle_solve(spec, ndim, Ar, Br, F, K, tol, vc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and 8 < want[1] < vc.MAX_LAUNCHES and want[1] % 8 == 0, want
    dA, dB, dF, dK = _dev(torch, A, B, F, K)
    dR = _nan_res(torch, kern, dt)
    kw = {"d_src": dF.data_ptr(), "d_coef": dK.data_ptr()}
    status, launches, r = kern.solve(dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), tol, vc.MAX_LAUNCHES, check_every=4, **kw)
    print(cid, "launches", launches, "residual", repr(r), "reference", want)
    assert status == 0 and launches == want[1], (status, launches, want)
    assert rc.same_bits(np.asarray(r, dt), want[2]) and kern.residual(dR.data_ptr()) == r
    assert bit_equal(dA.cpu().numpy(), Ar) and bit_equal(dB.cpu().numpy(), Br) and bit_equal(dK.cpu().numpy(), K)
    # run() and run_timed() and the gold loop through the operand block
    dA, dB = _dev(torch, A, B)
    assert kern.run(dA.data_ptr(), dB.data_ptr(), iterations=8, d_res=dR.data_ptr(), **kw) == 8
    Ar, Br = A.copy(), B.copy()
    ref = vc.oracle_solve(spec, ndim, Ar, Br, F, K, 0.0, 8, 4)
    assert rc.same_bits(np.asarray(kern.residual(dR.data_ptr()), dt), ref[2]) and bit_equal(dA.cpu().numpy(), Ar)
    n, ms = kern.run_timed(dA.data_ptr(), dB.data_ptr(), iterations=4, warmup=0, d_res=dR.data_ptr(), **kw)
    assert n == 4 and ms > 0
    dA, dB = _dev(torch, A, B)
    assert kern.run(dA.data_ptr(), dB.data_ptr(), iterations=8, gold=True, **kw) == 8
    torch.cuda.synchronize()
    assert bit_equal(dA.cpu().numpy(), Ar)


# ---- the operand block with coef set on old kinds of kernel, the emitted program -------------------------------------------------------
def test_operand_block_refuses_coef_on_old_kinds(torch_cuda):
    """drs_kernel_launch_ops with coef set on a plain, a --source, a --dirichlet, a --residual max and a --scale kernel: -2, nothing
    launched (the arrays stay as they were); with coef NULL the same block runs."""
    import dirichlet_cases as dc
    import drstencil_amd as drs
    torch = torch_cuda
    L = drs.lib()
    cid, ndim, stc, opts = vc.EDGE[1]
    spec = oracle.Spec(stc, ndim, 1)
    for extra in ([], vc.SOURCE, vc.DIR, rc.RES, sc.SCALE):
        full = list(opts) + extra
        kern = drs.Kernel(full + [stc])
        A0, B0, F0, X, W = sc.inputs(spec, full)
        X = X if extra == vc.DIR else None
        W = W if extra == sc.SCALE else None
        dA, dB, dF, dX, dW = _dev(torch, A0, B0, F0, X, W)
        dR = _nan_res(torch, kern, A0.dtype)
        dK = torch.zeros((7,) + A0.shape, dtype=dA.dtype, device="cuda")
        ptr = lambda d: None if d is None else d.data_ptr()          # noqa: E731
        bad = ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands), ptr(dF), ptr(dR), ptr(dX), ptr(dW), dK.data_ptr()))
        assert L.drs_kernel_launch_ops(kern.h, dA.data_ptr(), dB.data_ptr(), bad, 0) == -2
        assert L.drs_kernel_run_ops(kern.h, dA.data_ptr(), dB.data_ptr(), bad, 2, 0, 0) == -2
        torch.cuda.synchronize()
        assert bit_equal(dA.cpu().numpy(), A0) and bit_equal(dB.cpu().numpy(), B0), extra
        good = ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands), ptr(dF), ptr(dR), ptr(dX), ptr(dW)))
        assert L.drs_kernel_launch_ops(kern.h, dA.data_ptr(), dB.data_ptr(), good, 0) == 0
        torch.cuda.synchronize()
        assert not bit_equal(dB.cpu().numpy(), B0), extra


def test_emitted_check_program(torch_cuda):
    """The prebuilt --check --varcoef program (periodic, order 2, source, varcoef): dr_ and gold_ run with the same coef and agree."""
    exe = vc.check_program_path()
    assert os.path.exists(exe), "build() makes it"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = p.stdout
    assert p.returncode == 0, (p.returncode, out[-1500:], p.stderr[-500:])
    assert "[Test] RMS Error: 0.000000e+00" in out and "differ" not in out, out[-1500:]
