"""The families of launch entry points of the C ABI on the MI355X: the plain, _src, _res and _fix entry points (include/drstencil_amd.h)
against the operand-block (_ops) ones, which take every kind of kernel.  From identical inputs a family's launch, gold launch, loop,
timed loop and run to tolerance leave both arrays and the whole residual array in the same bits as the _ops entry point, and return the
same counts and statuses.  Then the Python gold loop on a --residual max kernel, and the pair launch against two single launches.
Six small kernels, every one prebuilt by __graft_entry__.build(): nothing here starts hipcc.  Timed runs are compared for their launch
count and arrays only, never for their time."""
import ctypes
import os

import numpy as np
import pytest

import dirichlet_cases as dc
import gpu_cases
import residual_cases as rc
import source_cases
from drstencil_amd.multigpu import SlabPlan

pytestmark = pytest.mark.gpu


def _pair_args():
    """The --pair-launch 1 kernel of the middle rank of gpu_cases.SLAB_CASES[1] (3 ranks, fused step 2): both boundary views of 6 planes in
    one launch.  build() has written the view's spec into the kernel cache and compiled the kernel."""
    cid, world, stencil, ndim, opts = gpu_cases.SLAB_CASES[1]
    view = SlabPlan(70, 2, world, 1, 1).pair_view()          # t3_star has 70 planes; Halo 2 at step 2
    return opts + ["--pair-launch", "1", os.path.join(gpu_cases.ROOT, "drstencil_amd", "_kcache", "%s_slabL%d.stc" % (stencil, view))]


# (id, family, arguments, solve tolerance that is met).  plain: the 2D tile kernel; source: z-streaming, 9 stream blocks; residual: Jacobi on
# 18^3 in two stream blocks, which converges; residual + source: Jacobi for Poisson's equation in 2D, which converges; dirichlet + source +
# residual: the wave stencil (its taps sum to 2: the iteration grows, so the tolerance that is met is a generous one); pair: a slab view, fused step 2
CASES = [
    ("plain_2d", "plain", rc.KNOBS[6][3] + [rc.KNOBS[6][2]], None),
    ("source_3d", "src", source_cases.SMALL[0][3] + [source_cases.SMALL[0][2]], None),
    ("residual_3d", "res", rc.with_res(rc.SOLVE[0][3]) + [rc.SOLVE[0][2]], 1e-3),
    ("residual_source_2d", "res", rc.with_res(rc.POISSON2[3]) + [rc.POISSON2[2]], 1e-6),
    ("dirichlet_source_residual_3d", "fix", dc.with_fix(dc.RES_MODES[1][3]) + [dc.RES_MODES[1][2]], 1e30),
    ("pair_3d", "plain", _pair_args(), None),
]
ITERATIONS = 6


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")          # a cache miss is an error, not a hipcc run
    return torch


class Problem:
    """A kernel, its inputs on the host and its read-only arrays on the device."""

    def __init__(self, torch, args):
        import drstencil_amd as drs
        self.torch, self.kern = torch, drs.Kernel(args)
        i = self.kern.info
        shape = (i["L"], i["M"], i["N"]) if i["ndim"] == 3 else (i["M"], i["N"])
        self.dt = np.float32 if i["dtype"] == "fp32" else np.float64
        r = np.random.default_rng(5)
        self.A0, self.B0 = r.random(shape).astype(self.dt), r.random(shape).astype(self.dt)
        H = i["halo"]
        ring = np.ones(shape, bool)
        ring[tuple(slice(H, -H) for _ in shape)] = False
        self.A0[ring] = 0                                 # a ring of 0: the Jacobi iterations converge
        self.B0[ring] = 0
        self.src = torch.from_numpy((0.01 * r.random(shape)).astype(self.dt)).cuda() if self.kern.source else None
        self.fix = torch.from_numpy(dc.fix_pattern(shape, self.dt)).cuda() if self.kern.dirichlet else None
        self.p = {"src": self.src.data_ptr() if self.kern.source else None, "fix": self.fix.data_ptr() if self.kern.dirichlet else None}

    def fresh(self):
        """(A, B, res) on the device: the inputs, and the residual array filled with NaN (None without --residual max)."""
        t = self.torch
        n = self.kern.residual_elems
        return t.from_numpy(self.A0).cuda(), t.from_numpy(self.B0).cuda(), t.full((n,), float("nan"), dtype=t.from_numpy(self.A0).dtype, device="cuda") if n else None


def _bits(torch, x):
    return None if x is None else x.view(torch.int32 if x.element_size() == 4 else torch.int64)


def _same(torch, what, prob, legacy, ops):
    """Both calls from the problem's inputs: the same return value, A, B and the whole of d_res in the same bits.  Returns that value."""
    out = []
    for call in (legacy, ops):
        A, B, R = prob.fresh()
        rc_ = call(A.data_ptr(), B.data_ptr(), R.data_ptr() if R is not None else None)
        torch.cuda.synchronize()
        out.append((rc_, A, B, R))
    (r0, A0, B0, R0), (r1, A1, B1, R1) = out
    print(what, "returned", r0, r1)
    assert r0 == r1, (what, r0, r1)
    assert torch.equal(_bits(torch, A0), _bits(torch, A1)) and torch.equal(_bits(torch, B0), _bits(torch, B1)), what
    assert R0 is None or torch.equal(_bits(torch, R0), _bits(torch, R1)), (what, "d_res")
    assert not torch.equal(_bits(torch, A0), _bits(torch, prob.fresh()[0])) or not torch.equal(_bits(torch, B0), _bits(torch, prob.fresh()[1])), (what, "nothing ran")
    return r0


def _block(p, res, gold=False):
    import drstencil_amd as drs
    return ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands), p["src"], None if gold else res, p["fix"], None, None))


def _legacy(L, fam, h, p, gold_src):
    """The family's entry points as calls of (a, b, res): launch, gold, run(gold), timed and solve where the family has them."""
    s, x = p["src"], p["fix"]
    ms = ctypes.c_float()
    n, r = ctypes.c_int(), ctypes.c_double()
    if fam == "plain":
        return {"launch": lambda a, b, R: L.drs_kernel_launch(h, a, b, 0), "gold": lambda a, b, R: L.drs_kernel_launch_gold(h, a, b, 0),
                "run": lambda g: lambda a, b, R: L.drs_kernel_run(h, a, b, ITERATIONS, g, 0),
                "timed": lambda a, b, R: L.drs_kernel_run_timed(h, a, b, ITERATIONS, 1, 0, ms)}
    if fam == "src":
        return {"launch": lambda a, b, R: L.drs_kernel_launch_src(h, a, b, s, 0), "gold": lambda a, b, R: L.drs_kernel_launch_gold_src(h, a, b, s, 0),
                "run": lambda g: lambda a, b, R: L.drs_kernel_run_src(h, a, b, s, ITERATIONS, g, 0),
                "timed": lambda a, b, R: L.drs_kernel_run_timed_src(h, a, b, s, ITERATIONS, 1, 0, ms)}
    if fam == "res":      # the gold kernel keeps its entry point, and the family has no gold loop
        return {"launch": lambda a, b, R: L.drs_kernel_launch_res(h, a, b, s, R, 0),
                "gold": (lambda a, b, R: L.drs_kernel_launch_gold_src(h, a, b, s, 0)) if gold_src else (lambda a, b, R: L.drs_kernel_launch_gold(h, a, b, 0)),
                "run": lambda g: None if g else lambda a, b, R: L.drs_kernel_run_res(h, a, b, s, R, ITERATIONS, 0),
                "timed": lambda a, b, R: L.drs_kernel_run_timed_res(h, a, b, s, R, ITERATIONS, 1, 0, ms),
                "solve": lambda tol, mx, ev: lambda a, b, R: (L.drs_kernel_solve(h, a, b, s, R, tol, mx, ev, 0, ctypes.byref(n), ctypes.byref(r)), n.value, np.float64(r.value).tobytes())}
    return {"launch": lambda a, b, R: L.drs_kernel_launch_fix(h, a, b, s, R, x, 0), "gold": lambda a, b, R: L.drs_kernel_launch_gold_fix(h, a, b, s, x, 0),
            "run": lambda g: lambda a, b, R: L.drs_kernel_run_fix(h, a, b, s, R, x, ITERATIONS, g, 0),
            "timed": lambda a, b, R: L.drs_kernel_run_timed_fix(h, a, b, s, R, x, ITERATIONS, 1, 0, ms),
            "solve": lambda tol, mx, ev: lambda a, b, R: (L.drs_kernel_solve_fix(h, a, b, s, R, x, tol, mx, ev, 0, ctypes.byref(n), ctypes.byref(r)), n.value, np.float64(r.value).tobytes())}


def _ops(L, h, p):
    ms = ctypes.c_float()
    n, r = ctypes.c_int(), ctypes.c_double()
    return {"launch": lambda a, b, R: L.drs_kernel_launch_ops(h, a, b, _block(p, R), 0), "gold": lambda a, b, R: L.drs_kernel_launch_gold_ops(h, a, b, _block(p, R, True), 0),
            "run": lambda g: lambda a, b, R: L.drs_kernel_run_ops(h, a, b, _block(p, R, bool(g)), ITERATIONS, g, 0),
            "timed": lambda a, b, R: L.drs_kernel_run_timed_ops(h, a, b, _block(p, R), ITERATIONS, 1, 0, ms),
            "solve": lambda tol, mx, ev: lambda a, b, R: (L.drs_kernel_solve_ops(h, a, b, _block(p, R), tol, mx, ev, 0, ctypes.byref(n), ctypes.byref(r)), n.value, np.float64(r.value).tobytes())}


@pytest.mark.parametrize("cid,fam,args,tol", CASES, ids=[c[0] for c in CASES])
def test_family_equals_operand_block(torch_cuda, cid, fam, args, tol):
    import drstencil_amd as drs
    torch = torch_cuda
    prob = Problem(torch, args)
    k, L = prob.kern, drs.lib()
    legacy, ops = _legacy(L, fam, k.h, prob.p, k.source), _ops(L, k.h, prob.p)
    loop = 2 * -(-ITERATIONS // (2 * k.info["step"]))
    assert _same(torch, cid + " launch", prob, legacy["launch"], ops["launch"]) == 0
    assert _same(torch, cid + " launch_gold", prob, legacy["gold"], ops["gold"]) == 0
    for g in (0, 1):
        if legacy["run"](g) is not None:
            assert _same(torch, cid + " run gold=%d" % g, prob, legacy["run"](g), ops["run"](g)) == loop
    assert _same(torch, cid + " run_timed", prob, legacy["timed"], ops["timed"]) == loop
    if "solve" in legacy:
        # a tolerance that is met; an odd max_launches, never met; a look at the residual after every pair
        status, launches, _ = _same(torch, cid + " solve", prob, legacy["solve"](tol, rc.MAX_LAUNCHES, 8), ops["solve"](tol, rc.MAX_LAUNCHES, 8))
        assert status == 0 and 0 < launches < rc.MAX_LAUNCHES and launches % 16 == 0
        assert _same(torch, cid + " solve max_launches=17", prob, legacy["solve"](0.0, 17, 8), ops["solve"](0.0, 17, 8))[:2] == (1, 16)
        status, every1, _ = _same(torch, cid + " solve check_every=1", prob, legacy["solve"](tol, rc.MAX_LAUNCHES, 1), ops["solve"](tol, rc.MAX_LAUNCHES, 1))
        assert status == 0 and launches - 16 < every1 <= launches and every1 % 2 == 0


def test_python_gold_loop_on_residual_kernel(torch_cuda):
    """Kernel.run(gold=True) on a --residual max kernel, one call of drs_kernel_run_ops, equals a loop of Kernel.launch_gold."""
    torch = torch_cuda
    prob = Problem(torch, CASES[2][2])
    k = prob.kern
    assert k.residual_elems and not k.source
    A, B, R = prob.fresh()
    assert k.run(A.data_ptr(), B.data_ptr(), ITERATIONS, gold=True) == ITERATIONS
    Al, Bl, _ = prob.fresh()
    for _ in range(ITERATIONS // 2):
        k.launch_gold(Al.data_ptr(), Bl.data_ptr())
        k.launch_gold(Bl.data_ptr(), Al.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch, A), _bits(torch, Al)) and torch.equal(_bits(torch, B), _bits(torch, Bl))
    assert bool(torch.isnan(R).all())                     # the gold kernel computes no residual
    assert not torch.equal(_bits(torch, A), _bits(torch, prob.fresh()[0]))
    with pytest.raises(ValueError, match="the gold kernel computes no residual"):
        k.run(A.data_ptr(), B.data_ptr(), ITERATIONS, gold=True, d_res=R.data_ptr())


def test_pair_launch_equals_two_launches(torch_cuda):
    """drs_kernel_launch_pair on two (in, out) pairs: each output in the bits of a single drs_kernel_launch on that pair."""
    import drstencil_amd as drs
    torch = torch_cuda
    prob = Problem(torch, CASES[5][2])
    k, L = prob.kern, drs.lib()
    in0, in1, _ = prob.fresh()
    out0, out1, want0, want1 = (torch.zeros_like(in0) for _ in range(4))
    assert L.drs_kernel_launch_pair(k.h, in0.data_ptr(), out0.data_ptr(), in1.data_ptr(), out1.data_ptr(), 0) == 0
    assert L.drs_kernel_launch(k.h, in0.data_ptr(), want0.data_ptr(), 0) == 0 and L.drs_kernel_launch(k.h, in1.data_ptr(), want1.data_ptr(), 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch, out0), _bits(torch, want0)) and torch.equal(_bits(torch, out1), _bits(torch, want1))
    assert bool((out0 != 0).any()) and not torch.equal(_bits(torch, out0), _bits(torch, out1))
    assert L.drs_kernel_launch_pair(Problem(torch, CASES[0][2]).kern.h, 1, 2, 3, 4, 0) == -2      # a kernel without --pair-launch 1
