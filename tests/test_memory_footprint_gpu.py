"""The memory contract of a launch, on the MI355X: a launch reads only read_mask cells of its input, writes only the interior of its
output (periodic: plus the input's ring) and touches no byte outside the two arrays.

HOW THIS IS CHECKED, AND HOW NOT.  On the GPU an access outside an allocation is a fault, and a fault can take the device down for
everybody on it, so these tests NEVER place an array at the edge of an allocation.  Every case allocates ONE torch.uint8 arena
`[G | A | G | B | G]` and carves A and B out of it as views: an overrun of up to G bytes lands in memory the test owns and is
DETECTED (the guard bands are compared with their saved clones), not trapped.  Do not "improve" this with edge placement, guard
pages or anything else that turns an overrun into a fault; placement against inaccessible pages is what the CPU twin does
(tests/test_memory_footprint_cpu.py, emulated kernels in child processes).  G is the larger of 1 MiB and two planes of the grid
(2D: two blocks of sn + 2 Halo rows), rounded up to 256 bytes -- a condition, not a measurement: the largest overrun the emitter
can plausibly produce is a prefetch of a whole plane past the end.

Per case and arena layout (A and B 256-byte aligned; both shifted by 16 bytes, the minimum the 16-byte vector paths may assume; for
kernels with element-wide accesses, N * sizeof % 16 != 0, also shifted by one element):
  run 1: guards = a finite bit pattern, A = seeded data, B = another seeded fill, the spec's run through Kernel.run: guards
         unchanged, A and B equal the oracle (bit for bit; the project's bars for on-chip pipelines), B's ring is its initial fill;
  run 2: guards = NaN, A = poison(A0) (NaN in every cell the stencil does not read), B = all NaN, ONE Kernel.launch: guards
         unchanged, B's interior NaN-free and equal to the oracle's sweep of the poisoned input, B's ring and A bit for bit unchanged
         (periodic: A's NaN ring comes back as the images of its interior).
Results must be bit-identical between layouts.  Every kernel comes from the cache (DRS_NO_COMPILE=1): a miss is a failure, not a
hipcc run after HIP is up.  The tests launch in-process, like the parity tests; they start no child process and no profiler."""
import os

import numpy as np
import pytest

import oracle
from footprint import bit_equal, int_view, interior_slices, is_poison, nan_filled, poison, poison_periodic, read_mask_torch, ring_mask
from gpu_cases import SLAB_CASES, SMALL
from gpu_cases import stc as stcp
from periodic_cases import SMALL as PERIODIC_SMALL
from periodic_cases import full_cases as periodic_full_cases
from periodic_cases import host_wrap, oracle_periodic_run

pytestmark = pytest.mark.gpu
REL_TOL = {"fp32": 1e-6, "fp64": 1e-12}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCACHE = os.path.join(ROOT, "drstencil_amd", "_kcache")
FINITE_BYTE = 0x3C        # 0x3C3C3C3C = 0.0115 (fp32), 0x3C3C... = 1.5e-18 (fp64): finite at any alignment
NAN_BYTE = 0xFF           # 0xFFFFFFFF / 0xFFFF...: a NaN at any alignment


@pytest.fixture
def torch_cuda(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    monkeypatch.setenv("DRS_NO_COMPILE", "1")
    return torch


def _dtype(opts):
    return "fp32" if "fp32" in opts else "fp64"


def _step(opts):
    return int(opts[opts.index("--step") + 1]) if "--step" in opts else 1


def _up(x, a):
    return -(-x // a) * a


def guard_bytes(info):
    """The larger of 1 MiB and two planes of the grid (2D: two blocks of sn + 2 Halo rows), rounded up to 256 bytes."""
    size = 4 if info["dtype"] == "fp32" else 8
    if info["ndim"] == 3:
        two = 2 * info["M"] * info["N"] * size
    else:
        rows = max(info.get("sn", 1), info.get("tile_owned_rows", 1)) + 2 * info["halo"]
        two = 2 * rows * info["N"] * size
    return _up(max(1 << 20, two), 256)


def layouts(info):
    size = 4 if info["dtype"] == "fp32" else 8
    out = [("aligned256", 0), ("shift16", 16)]
    if (info["N"] * size) % 16:
        out.append(("shift_element", size))
    return out


class Arena:
    """[G | array | G | array | ... | G] in one uint8 allocation; every array `shift` bytes past a multiple of 256."""

    def __init__(self, torch, nbytes, G, shift, count=2):
        assert G % 256 == 0 and 0 <= shift < 256 and G >= (1 << 20)
        self.torch, self.nbytes = torch, nbytes
        stride = G + _up(nbytes + shift, 256)
        self.buf = torch.empty(count * stride + G, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.offs = [k * stride + G + shift for k in range(count)]
        edges = [0]
        for o in self.offs:
            edges += [o, o + nbytes]
        edges.append(self.buf.numel())
        self.guards = [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2)]
        assert len(self.guards) == count + 1 and all(b - a >= G - 256 for a, b in self.guards)
        # every array strictly inside the allocation, a guard band of (about) G bytes on both sides: never at an edge
        assert all(o >= G and o + nbytes + G - 256 <= self.buf.numel() for o in self.offs)

    def ptr(self, k):
        return self.buf.data_ptr() + self.offs[k]

    def fill_guards(self, byte):
        for a, b in self.guards:
            self.buf[a:b].fill_(byte)
        self.saved = [self.buf[a:b].clone() for a, b in self.guards]

    def guards_intact(self):
        return [self.torch.equal(self.buf[a:b], s) for (a, b), s in zip(self.guards, self.saved)]

    def put(self, k, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes == self.nbytes
        self.buf[self.offs[k]:self.offs[k] + self.nbytes].copy_(self.torch.from_numpy(host.view(np.uint8).reshape(-1)))

    def get(self, k, dtype, shape):
        return self.buf[self.offs[k]:self.offs[k] + self.nbytes].cpu().numpy().view(dtype).reshape(shape)


def _compare(cid, spec, got, ref, bar):
    if bar is None:
        assert bit_equal(got, ref), (cid, "not bit-exact", oracle.check(spec, got, ref))
    else:
        m = oracle.check(spec, got, ref)
        assert m["max_rel"] <= bar, (cid, m)
        ring = ring_mask(got.shape, spec.halo)
        assert bit_equal(got[ring], ref[ring]), (cid, "ring")


def check_small(torch, cid, kern, spec, opts):
    """Both runs of the module docstring on every arena layout of one kernel."""
    info = kern.info
    dt = _dtype(opts)
    npdt = np.dtype(np.float32 if dt == "fp32" else np.float64)
    periodic = kern.periodic
    pipeline = info.get("stages", 1) > 1
    bar = REL_TOL[dt] if pipeline else None
    H = spec.halo
    assert info["halo"] == H and tuple(spec.shape) == ((info["L"], info["M"], info["N"]) if info["ndim"] == 3 else (info["M"], info["N"]))
    shape = tuple(spec.shape)
    nbytes = int(np.prod(shape)) * npdt.itemsize
    ring = ring_mask(shape, H)
    inner = interior_slices(shape, H)
    A0 = oracle.fill_random(shape, npdt)
    B0 = oracle.fill_random(shape, npdt, seed=9)
    A_ref, B_ref = A0.copy(), B0.copy()
    n_ref = oracle_periodic_run(spec, A_ref, B_ref) if periodic else oracle.run(spec, A_ref, B_ref, contract=1)
    P = poison_periodic(A0, spec) if periodic else poison(A0, spec)
    P_after = host_wrap(P.copy(), H) if periodic else P
    Bp_ref = nan_filled(shape, npdt)
    oracle.sweep(spec, P_after, Bp_ref, contract=1)
    assert not np.isnan(Bp_ref[inner]).any()
    first = None
    G = guard_bytes(info)
    for lid, shift in layouts(info):
        ar = Arena(torch, nbytes, G, shift)
        assert ar.ptr(0) % 16 == shift % 16 and ar.ptr(1) % 16 == shift % 16
        # run 1
        ar.fill_guards(FINITE_BYTE)
        ar.put(0, A0)
        ar.put(1, B0)
        n = kern.run(ar.ptr(0), ar.ptr(1))
        torch.cuda.synchronize()
        assert ar.guards_intact() == [True] * 3, (cid, lid, "run: a guard band was written [before A, between, behind B]", ar.guards_intact())
        A, B = ar.get(0, npdt, shape), ar.get(1, npdt, shape)
        assert n == n_ref
        _compare((cid, lid, "A"), spec, A, A_ref, bar)
        if periodic and pipeline:
            assert oracle.check(spec, B, B_ref)["max_rel"] <= bar, (cid, lid)
            assert bit_equal(B, host_wrap(B.copy(), H)), (cid, lid)
        else:
            _compare((cid, lid, "B"), spec, B, B_ref, bar)
            if not periodic:
                assert bit_equal(B[ring], B0[ring]), (cid, lid, "B's ring is not its initial fill")
        # run 2
        ar.fill_guards(NAN_BYTE)
        ar.put(0, P)
        ar.put(1, nan_filled(shape, npdt))
        kern.launch(ar.ptr(0), ar.ptr(1))
        torch.cuda.synchronize()
        assert ar.guards_intact() == [True] * 3, (cid, lid, "poison launch: a guard band was written", ar.guards_intact())
        Ap, Bp = ar.get(0, npdt, shape), ar.get(1, npdt, shape)
        assert not np.isnan(Bp[inner]).any(), (cid, lid, "%d NaN reached the output" % int(np.isnan(Bp[inner]).sum()))
        assert is_poison(Bp)[ring].all(), (cid, lid, "the output's ring was written")
        assert bit_equal(Ap, P_after), (cid, lid, "the input was written")
        if bar is None:
            assert bit_equal(Bp[inner], Bp_ref[inner]), (cid, lid)
        else:
            assert oracle.check(spec, Bp, Bp_ref)["max_rel"] <= bar, (cid, lid)
        if first is None:
            first = (A, B, Bp)
        else:
            assert bit_equal(A, first[0]) and bit_equal(B, first[1]) and bit_equal(Bp, first[2]), (cid, lid, "results depend on the placement")
        del ar


@pytest.mark.parametrize("cid,ndim,stc,opts", SMALL, ids=[c[0] for c in SMALL])
def test_footprint_small(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    check_small(torch_cuda, cid, drs.Kernel(opts + [stc]), oracle.Spec(stc, ndim, _step(opts)), opts)


@pytest.mark.parametrize("cid,ndim,stc,opts", PERIODIC_SMALL, ids=[c[0] for c in PERIODIC_SMALL])
def test_footprint_periodic_small(torch_cuda, cid, ndim, stc, opts):
    import drstencil_amd as drs
    kern = drs.Kernel(opts + [stc])
    assert kern.periodic
    check_small(torch_cuda, cid, kern, oracle.Spec(stc, ndim, _step(opts)), opts)


def _slab_view_lengths(world, stencil, ndim, opts):
    import drstencil_amd as drs
    from drstencil_amd.multigpu import SlabPlan
    spec = drs.Spec(stcp(stencil), ndim, _step(opts))
    cut = spec.dims[0] if ndim == 3 else spec.dims[1]
    return sorted({n for r in range(world) for every in (1, 2) for n in SlabPlan(cut, spec.halo, world, r, every).views()})


@pytest.mark.parametrize("cid,world,stencil,ndim,opts", SLAB_CASES, ids=[c[0] for c in SLAB_CASES])
def test_footprint_slab_views(torch_cuda, cid, world, stencil, ndim, opts):
    """The slab-view kernels of every rank and both exchange modes, each on an arena holding exactly its view: what the last rank's
    kernels get, whose view ends where the array ends."""
    from drstencil_amd.multigpu import HipSweep
    sweep = HipSweep(stcp(stencil), opts, KCACHE)
    lengths = _slab_view_lengths(world, stencil, ndim, opts)
    assert lengths
    for n in lengths:
        kern = sweep.kernel(n)
        assert (kern.info["L"] if ndim == 3 else kern.info["M"]) == n
        check_small(torch_cuda, "%s_view%d" % (cid, n), kern, oracle.Spec(kern.args[-1], ndim, _step(opts)), opts)
    print("slab views of %s: %s" % (cid, lengths))


@pytest.mark.parametrize("every", [1, 2])
def test_footprint_pair_launch(torch_cuda, every):
    """The dr2_ pair launch of the C4 slab run's middle ranks (bench.slab_options("c4", 4)) with four guarded arrays."""
    import bench
    from drstencil_amd.multigpu import HipSweep, SlabPlan
    torch = torch_cuda
    opts = bench.slab_options("c4", 4)
    n = SlabPlan(1024, 2, 4, 1, every).pair_view()
    assert n
    kern = HipSweep(bench.WORKLOADS["c4"]["stc"], opts, KCACHE).kernel(n, pair=True)
    info = kern.info
    shape = (info["L"], info["M"], info["N"])
    assert shape == (n, 1024, 1024)
    spec = oracle.Spec(kern.args[-1], 3, _step(opts))
    H = spec.halo
    inner, ring = interior_slices(shape, H), ring_mask(shape, H)
    a0 = oracle.fill_random(shape, np.float32)
    a1 = oracle.fill_random(shape, np.float32, seed=3)
    fill = oracle.fill_random(shape, np.float32, seed=9)
    first = {}
    for lid, shift in layouts(info):
        ar = Arena(torch, a0.nbytes, guard_bytes(info), shift, count=4)
        for poisoned in (False, True):
            ins = [poison(a, spec) for a in (a0, a1)] if poisoned else [a0, a1]
            out0 = nan_filled(shape, np.float32) if poisoned else fill
            ar.fill_guards(NAN_BYTE if poisoned else FINITE_BYTE)
            for k, h in enumerate((ins[0], out0, ins[1], out0)):
                ar.put(k, h)
            kern.launch_pair(ar.ptr(0), ar.ptr(1), ar.ptr(2), ar.ptr(3))
            torch.cuda.synchronize()
            assert ar.guards_intact() == [True] * 5, (lid, poisoned, ar.guards_intact())
            outs = []
            for k in (0, 1):
                ref = out0.copy()
                oracle.sweep(spec, ins[k], ref, contract=1)
                got_in, got = ar.get(2 * k, np.float32, shape), ar.get(2 * k + 1, np.float32, shape)
                assert bit_equal(got_in, ins[k]), (lid, poisoned, k, "the input was written")
                assert not np.isnan(got[inner]).any(), (lid, poisoned, k)
                assert bit_equal(got[ring], out0[ring]), (lid, poisoned, k, "the output's ring was written")
                assert bit_equal(got, ref), (lid, poisoned, k)
                outs.append(got)
            assert not bit_equal(outs[0], outs[1])
            if poisoned not in first:
                first[poisoned] = outs
            else:
                assert all(bit_equal(x, y) for x, y in zip(outs, first[poisoned])), (lid, "results depend on the placement")
        del ar


def _full_cases():
    import bench
    w = bench.WORKLOADS
    return [("C4_headline", "c4", bench.TUNED["c4"], w["c4"]["stc"]),
            ("C4_fp64_temporal4", "c4f64", bench.TEMPORAL4["c4f64"], w["c4f64"]["stc"]),
            ("C2_tile", "c2", bench.TUNED["c2"], w["c2"]["stc"]),
            ("C5_fp64", "c5", bench.TUNED["c5"], w["c5"]["stc"]),
            ("C4_headline_periodic", "c4", periodic_full_cases()[0][3], periodic_full_cases()[0][2])]


@pytest.mark.parametrize("cid,workload,opts,stc", _full_cases(), ids=[c[0] for c in _full_cases()])
def test_footprint_full_size(torch_cuda, cid, workload, opts, stc):
    """BASELINE sizes, one launch each, guards + poison only (the values are tied to the oracle by test_full_size_properties and
    test_3d7pt_whole_grid_vs_oracle): byte offsets pass 2^32 here, so the 31-bit buffer-offset conditions of the emitter are actually
    exercised.  Guards NaN, A poisoned, B all NaN, everything compared on the device: guards unchanged, interior NaN-free, A unchanged
    (periodic: its NaN ring replaced by the images of the interior), and dr == gold kernel bit for bit on the poisoned input (within
    the project's bar for an on-chip pipeline) -- the gold kernel is one lane per point under an explicit interior guard."""
    import drstencil_amd as drs
    torch = torch_cuda
    kern = drs.Kernel(list(opts) + [stc])
    info = kern.info
    ndim = info["ndim"]
    dt = info["dtype"]
    tdt = torch.float32 if dt == "fp32" else torch.float64
    shape = (info["L"], info["M"], info["N"]) if ndim == 3 else (info["M"], info["N"])
    spec = oracle.Spec(stc, ndim, info["step"])
    H = spec.halo
    assert H == info["halo"] and tuple(spec.shape) == shape
    nbytes = int(np.prod(shape)) * (4 if dt == "fp32" else 8)
    inner = interior_slices(shape, H)
    ar = Arena(torch, nbytes, guard_bytes(info), 0)
    A = ar.buf[ar.offs[0]:ar.offs[0] + nbytes].view(tdt).view(shape)
    B = ar.buf[ar.offs[1]:ar.offs[1] + nbytes].view(tdt).view(shape)
    ar.fill_guards(NAN_BYTE)
    g = torch.Generator(device="cuda").manual_seed(2024)
    A.copy_(torch.rand(shape, dtype=tdt, device="cuda", generator=g))
    nan = float("nan")
    if kern.periodic:
        for ax in range(ndim):                   # the whole ring
            A.narrow(ax, 0, H).fill_(nan)
            A.narrow(ax, shape[ax] - H, H).fill_(nan)
    else:
        mask = read_mask_torch(torch, spec, "cuda")
        A.masked_fill_(~mask, nan)               # (a box reads every cell: nothing to poison but the output and the guards)
        del mask
    P = A.clone()
    expect = host_wrap(P.clone(), H) if kern.periodic else P         # slice assignments: the same function on a device tensor
    assert not kern.periodic or not torch.isnan(expect).any()
    B.fill_(nan)
    ring_before = int_view(torch, B).clone()
    ring_before[inner] = 0
    out = {}
    for which in ("dr", "gold"):                 # the gold kernel in the same arena: no array at the edge of an allocation, ever
        A.copy_(P)
        B.fill_(nan)
        (kern.launch if which == "dr" else kern.launch_gold)(A.data_ptr(), B.data_ptr())
        torch.cuda.synchronize()
        assert ar.guards_intact() == [True] * 3, (cid, which, "a guard band was written [before A, between, behind B]", ar.guards_intact())
        assert not torch.isnan(B[inner]).any(), (cid, which, "%d NaN reached the output" % int(torch.isnan(B[inner]).sum()))
        assert torch.equal(int_view(torch, A), int_view(torch, expect)), (cid, which, "the input was written")
        ring_after = int_view(torch, B).clone()   # the output's ring: still the NaN it was
        ring_after[inner] = 0
        assert torch.equal(ring_after, ring_before), (cid, which, "the output's ring was written")
        del ring_after
        out[which] = B[inner].clone()
    if info.get("stages", 1) > 1:
        got, ref = out["dr"].double(), out["gold"].double()
        rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())
        print("%s: dr vs gold max_rel %.3g" % (cid, rel))
        assert rel <= REL_TOL[dt], (cid, rel)
    else:
        assert torch.equal(out["dr"], out["gold"]), cid
