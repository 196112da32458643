"""The memory contract of a launch, on the CPU: emitted kernels under the emulation (tests/emu) with both arrays placed flush
against inaccessible pages -- once with the last byte against the trailing page, once with the first byte behind the leading one --
so that a load or store outside `[base, base + L*M*N*sizeof)` is a SIGSEGV instead of an access to slack nobody looks at; and with
NaN in every cell of the input that the stencil does not read and in all of the output, so that a value fetched from the wrong
place and masked by arithmetic (`0 * x`) instead of by a select shows up in the result.  Every case runs in a child process
(tests/footprint_child.py).  The value tests of the same kernels are tests/test_emulated_kernels.py and tests/test_periodic_cpu.py;
the GPU side is tests/test_memory_footprint_gpu.py.

The harness itself is checked first: a hand-written plugin (tests/native/footprint_selftest.c) with switchable defects must be
reported for each of them and pass without."""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import oracle
from emu_util import build_emulated
from footprint import bit_equal, int_view, is_poison, nan_filled, poison, read_mask, read_mask_torch, ring_mask
from helpers import write_stc
from periodic_cases import PERIODIC
from test_emulated_kernels import ASYM, DMA, EDGE, RACE, REUSE, VARIANTS, _emulated_fuzz_jobs, _mg, _random_shape_jobs
from test_periodic_cpu import RUNS, SHAPES, WRAP_CASES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD = os.path.join(HERE, "footprint_child.py")
PLACEMENTS = ["end", "start"]
# the sampled lists run end-flush only: with both placements this file more than doubled the wall time of the not-gpu suite, and
# the hand-picked lists (both placements) already hold every staging, store and schedule path the samples draw from
SAMPLED_PLACEMENTS = ["end"]


class ChildResult:
    def __init__(self, cid, proc):
        self.cid, self.returncode, self.stdout, self.stderr = cid, proc.returncode, proc.stdout, proc.stderr
        lines = proc.stdout.splitlines()
        phases = [ln[6:] for ln in lines if ln.startswith("PHASE ")]
        fails = [ln[5:] for ln in lines if ln.startswith("FAIL ")]
        self.phase = phases[-1] if phases else "(none announced)"
        self.signal = signal.Signals(-proc.returncode).name if proc.returncode < 0 else None
        self.kind = "out_of_bounds" if self.signal == "SIGSEGV" else fails[-1].split(":")[0] if fails else None
        self.ok = proc.returncode == 0 and bool(lines) and lines[-1] == "DONE"
        if self.ok:
            self.message = "ok"
        elif self.signal == "SIGSEGV":
            self.message = "%s: out of bounds: SIGSEGV on an access outside the arrays, during phase '%s'" % (cid, self.phase)
        elif self.signal:
            self.message = "%s: killed by %s during phase '%s'" % (cid, self.signal, self.phase)
        else:
            self.message = "%s: exit status %d during phase '%s': %s\n%s" % (cid, proc.returncode, self.phase, "; ".join(fails) or "no FAIL line", proc.stderr[-1500:])


def run_child(cid, tmp_path, job, env=None):
    path = os.path.join(str(tmp_path), "job.json")
    with open(path, "w") as f:
        json.dump(job, f)
    e = dict(os.environ)
    e.pop("EMU_ORDER", None)
    e.pop("FOOTPRINT_DEFECT", None)
    e.update(env or {})
    return ChildResult(cid, subprocess.run([sys.executable, CHILD, path], env=e, capture_output=True, text=True, timeout=1200))


def _step(opts):
    return int(opts[opts.index("--step") + 1]) if "--step" in opts else 1


def _sweep_job(lib, stc, opts, periodic=False, placements=PLACEMENTS):
    return dict(mode="sweep", so=lib._name, stc=stc, ndim=3 if "--3d" in opts else 2, step=_step(opts), dtype="float32" if "fp32" in opts else "float64",
                temporal="--temporal" in opts, periodic=periodic, placements=placements)


# ---- the helpers and the harness ------------------------------------------------------------------------------------------------------
def test_read_mask_and_poison(tmp_path):
    """read_mask is the union of the interior box shifted by every tap; poison() leaves exactly those cells and the oracle clean."""
    stc = str(tmp_path / "s.stc")
    write_stc(stc, 2, (1, 9, 12), 2, SHAPES["STAR2"][1])
    spec = oracle.Spec(stc, 2, 1)
    m = read_mask(spec)
    corners = np.zeros((9, 12), bool)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    assert np.array_equal(m, ~corners)                              # a star of reach 1 reads everything but the four corners
    spec2 = oracle.Spec(stc, 2, 2)                                  # fused twice: a diamond of reach 2, ring of width 2
    m2 = read_mask(spec2)
    assert not m2[0, 0] and not m2[0, 1] and not m2[1, 0] and m2[1, 1] and m2[0, 2] and m2[2, 0] and m2[2:-2, 2:-2].all()
    write_stc(stc, 2, (1, 9, 12), 2, [(0, 0, 0.5), (1, 0, 0.2), (0, 1, 0.3)])    # one-sided: nothing above, nothing to the left
    m3 = read_mask(oracle.Spec(stc, 2, 1))
    assert not m3[0].any() and not m3[:, 0].any() and m3[1:, 1:].sum() == m3.sum() and not m3[-1, -1] and m3[-1, -2] and m3[-2, -1]
    A0 = oracle.fill_random(spec.shape, np.float64)
    P = poison(A0, spec)
    assert is_poison(P)[corners].all() and bit_equal(P[~corners], A0[~corners]) and np.isnan(P).sum() == 4
    assert bit_equal(nan_filled((3,), np.float32), nan_filled((3,), np.float32)) and not np.array_equal(nan_filled((3,), np.float32), nan_filled((3,), np.float32))
    assert ring_mask((5, 6), 1).sum() == 30 - 12
    import torch
    for sp in (spec, spec2):
        assert np.array_equal(read_mask_torch(torch, sp, "cpu").numpy(), read_mask(sp))
    t = torch.from_numpy(nan_filled((4,), np.float64))
    assert torch.equal(int_view(torch, t), int_view(torch, t.clone())) and not torch.equal(t, t.clone())


SELFTEST_DIMS = (1, 9, 12)
DEFECTS = [
    # (FOOTPRINT_DEFECT, the kind the harness must report, the phase it must report it in)
    ("", None, None),
    ("read_past_end", "out_of_bounds", "end-flush dr ping-pong run"),
    ("write_before_start", "out_of_bounds", "start-flush dr ping-pong run"),
    ("nan_leak", "nan_leak", "end-flush dr poison launch"),
    ("ring_write", "ring_changed", "end-flush dr ping-pong run"),
]


@pytest.mark.parametrize("defect,kind,where", DEFECTS, ids=[d[0] or "defect_free" for d in DEFECTS])
def test_harness_reports_planted_defects(tmp_path, defect, kind, where):
    """Without this, "all green" below proves nothing about the harness: a plugin that reads one element past the end, writes one
    element before the start, lets an unread cell reach the output through 0 * x, or writes a ring cell is reported as such, and the
    same plugin without a defect passes.  (CPU only: the defects are host code in a child process.)"""
    stc = str(tmp_path / "selftest.stc")
    write_stc(stc, 2, SELFTEST_DIMS, 2, SHAPES["STAR2"][1])
    spec = oracle.Spec(stc, 2, 1)
    assert [(o[1:], c) for o, c in spec.points] == [((-1, 0), 0.2), ((0, -1), 0.25), ((0, 0), 0.3), ((0, 1), 0.15), ((1, 0), 0.1)]    # the plugin's table
    so = str(tmp_path / "selftest.so")
    subprocess.check_call(["cc", "-O1", "-std=gnu11", "-shared", "-fPIC", "-ffp-contract=off", "-DFP_M=%d" % SELFTEST_DIMS[1], "-DFP_N=%d" % SELFTEST_DIMS[2],
                           os.path.join(HERE, "native", "footprint_selftest.c"), "-o", so, "-lm"])
    job = dict(mode="sweep", so=so, stc=stc, ndim=2, step=1, dtype="float64", temporal=False, periodic=False, placements=PLACEMENTS)
    r = run_child("selftest_" + (defect or "clean"), tmp_path, job, env={"FOOTPRINT_DEFECT": defect})
    print(r.message)
    if kind is None:
        assert r.ok, r.message
        return
    assert not r.ok and r.kind == kind and r.phase == where, (r.message, r.stdout)
    if kind == "out_of_bounds":
        assert r.signal == "SIGSEGV" and "out of bounds" in r.message and where in r.message
    else:
        assert r.returncode == 1 and kind in r.message and r.signal is None


# ---- emitted kernels -------------------------------------------------------------------------------------------------------------------
HAND_PICKED = [(lst, c) for lst, cases in (("VARIANTS", VARIANTS), ("REUSE", REUSE), ("DMA", DMA), ("EDGE", EDGE), ("RACE", RACE), ("ASYM", ASYM)) for c in cases]


@pytest.mark.parametrize("lst,case", HAND_PICKED, ids=["%s-%s" % (lst, c[0]) for lst, c in HAND_PICKED])
def test_footprint_hand_picked(lst, case, tmp_path):
    """Every hand-picked emulator case of test_emulated_kernels.py: both placements, the whole run and the poisoned launch, the
    kernel and its gold kernel.  RACE cases run with the fibers in reverse order, as they do there.  No skips."""
    vid, ndim, pts, dims, opts = case
    stc = str(tmp_path / "k.stc")
    write_stc(stc, ndim, dims, 4, getattr(_mg(), pts) if isinstance(pts, str) else pts)
    lib = build_emulated(tmp_path, stc, opts)
    r = run_child("%s-%s" % (lst, vid), tmp_path, _sweep_job(lib, stc, opts), env={"EMU_ORDER": "reverse"} if lst == "RACE" else None)
    assert r.ok, r.message


@pytest.mark.parametrize("vid,ndim,pts,dims,opts,step", _emulated_fuzz_jobs(), ids=[j[0] for j in _emulated_fuzz_jobs()])
def test_footprint_sampled_fuzz(vid, ndim, pts, dims, opts, step, tmp_path):
    """The tuner-space sample of test_emulated_sampled_fuzz (skipped exactly where that test skips: the generator rejects it)."""
    stc = str(tmp_path / "f.stc")
    write_stc(stc, ndim, dims, 4, getattr(_mg(), pts))
    try:
        lib = build_emulated(tmp_path, stc, opts)
    except AssertionError as e:
        assert "Invalid configuration" in str(e) or "tile" in str(e) or "halo" in str(e), str(e)[-300:]
        pytest.skip("rejected by the generator")
    assert _step(opts) == step
    r = run_child(vid, tmp_path, _sweep_job(lib, stc, opts, placements=SAMPLED_PLACEMENTS))
    assert r.ok, r.message


@pytest.mark.parametrize("vid,ndim,pts,dims,opts", _random_shape_jobs(), ids=[j[0] for j in _random_shape_jobs()])
def test_footprint_random_shapes(vid, ndim, pts, dims, opts, tmp_path):
    """The random point sets of test_emulated_random_shapes: one-sided shapes, shapes without a centre, duplicate offsets -- where
    read_mask leaves the most cells unread (skipped exactly where that test skips)."""
    stc = str(tmp_path / "s.stc")
    write_stc(stc, ndim, dims, 4, pts)
    try:
        lib = build_emulated(tmp_path, stc, opts)
    except AssertionError as e:
        assert "No data to reuse" in str(e) or "Invalid configuration" in str(e), str(e)[-300:]
        pytest.skip("rejected by the generator like the reference would: " + str(e).strip().splitlines()[-1][:120])
    r = run_child(vid, tmp_path, _sweep_job(lib, stc, opts, placements=SAMPLED_PLACEMENTS))
    assert r.ok, r.message


@pytest.mark.parametrize("cid,shape,dims,opts", RUNS, ids=[c[0] for c in RUNS])
def test_footprint_periodic_runs(cid, shape, dims, opts, tmp_path):
    """--boundary periodic: the launch writes the input's ring (the wrap) and nothing else of it; a ring full of NaN comes back as
    the images of the interior and no NaN reaches the output."""
    ndim, pts = SHAPES[shape]
    stc = str(tmp_path / "p.stc")
    write_stc(stc, ndim, dims, 2 * _step(opts), pts)
    lib = build_emulated(tmp_path, stc, opts + PERIODIC)
    r = run_child(cid, tmp_path, _sweep_job(lib, stc, opts, periodic=True))
    assert r.ok, r.message


@pytest.mark.parametrize("cid,shape,dims,opts", WRAP_CASES, ids=[c[0] for c in WRAP_CASES])
def test_footprint_wrap_alone(cid, shape, dims, opts, tmp_path):
    """drs_plugin_wrap on a guarded array == np.pad(interior, Halo, "wrap"): 16-byte vector and element paths, minimum grids."""
    ndim, pts = SHAPES[shape]
    stc = str(tmp_path / "w.stc")
    write_stc(stc, ndim, dims, 4, pts)
    lib = build_emulated(tmp_path, stc, opts + PERIODIC)
    job = dict(mode="wrap", so=lib._name, shape=list(dims if ndim == 3 else dims[1:]), dtype="float32" if "fp32" in opts else "float64", placements=PLACEMENTS)
    r = run_child(cid, tmp_path, job)
    assert r.ok, r.message


def test_footprint_pair_launch(tmp_path):
    """The dr2_ pair launch of test_emulated_pair_launch with all four arrays guarded."""
    stc = str(tmp_path / "p.stc")
    write_stc(stc, 3, (9, 21, 140), 4, _mg().STAR3)
    opts = ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "4", "--pair-launch", "1", "--bx", "16", "--by", "4", "--block-merge-y", "2"]
    lib = build_emulated(tmp_path, stc, opts)
    job = dict(mode="pair", so=lib._name, stc=stc, ndim=3, step=2, dtype="float32", placements=PLACEMENTS)
    r = run_child("pair_launch", tmp_path, job)
    assert r.ok, r.message


SLAB_VIEWS = [
    # (id, base dims, world, options): the LAST rank's views, whose kernels run on an allocation that ends where the view ends
    ("3d_w2_step1", 3, (24, 17, 264), 2, ["--3d", "--dtype", "fp32", "--sn", "8"]),
    ("3d_w3_fused2_prefetch", 3, (36, 21, 300), 3, ["--3d", "--dtype", "fp32", "--step", "2", "--sn", "6", "--prefetch", "--uniform-loads", "1"]),
    ("2d_w2_stream_step2", 2, (1, 80, 268), 2, ["--dtype", "fp32", "--streaming", "--step", "2", "--sn", "9", "--prefetch"]),
]


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("cid,ndim,dims,world,opts", SLAB_VIEWS, ids=[c[0] for c in SLAB_VIEWS])
def test_footprint_slab_views(cid, ndim, dims, world, opts, every, tmp_path):
    """The slab situation: a kernel built for a view of n planes (rows in 2D), launched on a guarded allocation of exactly n planes --
    what HipSweep's view kernels get on the last rank, where the view ends where the array ends (and on the first, where it starts
    where the array starts: the other placement)."""
    from drstencil_amd.multigpu import SlabPlan, _write_view_stc
    base = str(tmp_path / "base.stc")
    write_stc(base, ndim, dims, 4, _mg().STAR3 if ndim == 3 else _mg().STAR2)
    step = _step(opts)
    spec = oracle.Spec(base, ndim, step)
    plan = SlabPlan(dims[0] if ndim == 3 else dims[1], spec.halo, world, world - 1, every)
    views = plan.views()
    assert views
    for n in views:
        stc = _write_view_stc(base, ndim, n, str(tmp_path), "slabL")
        lib = build_emulated(tmp_path, stc, opts)
        r = run_child("%s_view%d" % (cid, n), tmp_path, _sweep_job(lib, stc, opts))
        assert r.ok, r.message
