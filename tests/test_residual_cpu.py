"""--residual max (r = max |out - in| over the interior, fused into the sweep) without a GPU: the generator's option surface, the C ABI's
refusals, and the emitted kernels under the CPU emulation (tests/emu) in both fiber orders -- arrays bit for bit against the job's host
reference, r bit for bit against numpy's max(abs(out - in)), a planted maximum at corners and seams, poisoned inputs and a NaN-filled
residual array, IEEE special values, the memory contract flush against inaccessible pages, and the run to tolerance.

The case list is tests/residual_cases.py's, the one tests/test_residual_gpu.py runs on the GPU.  The knob cases on t3_star run that
stencil on smaller grids here (more than one tile and stream block, partial tiles), so that each takes seconds under the emulation; the
70 x 45 x 530 case with early-leaving workgroups keeps its size."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import drstencil_amd as drs
import oracle
import residual_cases as rc
from emu_util import DRSTENCIL
from gpu_cases import SMALL as GPU_SMALL
from helpers import write_stc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = os.path.join(ROOT, "benchmarks", "configs", "c4_3d7pt_star_1024.stc")
RES = rc.RES
# grids of the emulated knob cases: (L, M, N)
DIMS = {"prefetch_depth2": (19, 37, 264), "defer_stores": (13, 19, 264), "rows_pack": (21, 19, 264), "cyclic_merge_x2_fp64": (13, 19, 140),
        "loader_waves_fp64": (13, 19, 140), "store_mask_buffer": (13, 37, 264), "fused_step2_fp32": (21, 19, 264), "fused_step3_fp64": (17, 19, 140),
        "odd_elem_fp64": (13, 21, 135), "tile_2d_fp32": (1, 41, 268), "tile_2d_box9_fp64": (1, 41, 140), "stream_2d_fp32": (1, 61, 268),
        "stream_2d_dma_fp64": (1, 45, 140)}


def _cli(args, cwd):
    return subprocess.run([DRSTENCIL] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


def _small_stc(tmp_path, src, ndim, dims, name=None):
    pts = [tuple(off[3 - ndim:]) + (c,) for off, c in oracle.Spec(src, ndim, 1).points]
    path = os.path.join(str(tmp_path), (name or os.path.basename(src)[:-4]) + ".stc")
    write_stc(path, ndim, dims, 4, pts)
    return path


def _case_stc(tmp_path, cid, ndim, src):
    return _small_stc(tmp_path, src, ndim, DIMS[cid]) if cid in DIMS else shutil.copy(src, str(tmp_path))


def _info(src):
    return json.loads(re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', src).group(1).replace('\\"', '"'))


def _second_lib(lib, tmp_path, tag):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    cp = os.path.join(str(tmp_path), tag + "_" + os.path.basename(lib.so))
    shutil.copy(lib.so, cp)
    return rc.load_emulated(cp)


def _nan_res(lib, dt):
    return np.full(lib.residual_elems, np.nan, dt)


def _three_launches(lib, spec, ndim, opts, A0, B0, F0, what):
    """Three launches from (A0, B0, F0): after each, both arrays equal the host reference's in bits, r equals numpy's in bits (or both
    are NaN), and every element of the NaN-filled residual array has been overwritten."""
    A, B = A0.copy(), B0.copy()
    Ar, Br = A0.copy(), B0.copy()
    for t in range(3):
        s, d = (A, B) if t % 2 == 0 else (B, A)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        res = _nan_res(lib, A.dtype)
        assert lib.launch(s, d, F0, res) == 0
        want = rc.host_launch(spec, ndim, opts, sr, dr, F0)
        assert np.array_equal(A, Ar) and np.array_equal(B, Br), (what, t, int((A != Ar).sum()), int((B != Br).sum()))
        assert rc.same_bits(res[0], want), (what, t, res[0], want)
        assert not np.isnan(res).any(), (what, t, "partials not written", np.argwhere(np.isnan(res))[:4])
        assert np.isfinite(want) and want > 0


# ---- generator / CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_residual(tmp_path):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (10, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + RES + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "residual" not in p.stdout                                      # stdout stays the reference's protocol
    notes = [ln for ln in p.stderr.splitlines() if "residual" in ln]
    assert len(notes) == 1 and notes[0].startswith("drstencil: note: residual: a launch takes one more array of ")
    src = open(out).read()
    info = _info(src)
    assert info["residual"] == "max" and info["residual_elems"] == 1 + info["grid"]
    assert "// options: --3d --dtype fp32 --residual max" in src
    assert "const real_t* __restrict__ d_in, real_t* __restrict__ d_out, real_t* __restrict__ d_res)" in src
    assert "drs_plugin_launch_res(const void* in, void* out, const void* src, void* res, hipStream_t stream)" in src
    assert "drs_plugin_launch(" not in src and "drs_plugin_launch_gold(const void* in, void* out, hipStream_t stream)" in src
    assert "res_p (real_t* __restrict__ d_res)" in src and "atomic" not in src
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert "d_res" not in gold and "rmax" not in gold                      # the gold kernel computes no residual
    rc2, msg, src2 = drs.generate(["--3d", "--dtype", "fp32"] + RES + ["-o", out, stc])
    assert rc2 == 0 and src2 == src and "drstencil: note: residual:" in msg
    # with --source the same single entry point, and gold keeps the three-pointer one
    p = _cli(["--3d", "--dtype", "fp32", "--source"] + RES + ["-o", out, stc], tmp_path)
    src = open(out).read()
    assert p.returncode == 0 and "drs_plugin_launch_res(" in src and "drs_plugin_launch_src(" not in src and "drs_plugin_launch_gold_src(" in src
    assert "--residual <max>" in drs.generate(["--help"])[1]


@pytest.mark.parametrize("extra,stdout,reason", [
    (["--step", "2", "--temporal", "1"], "Invalid configuration!\n", "--residual cannot be combined with --temporal"),
    (["--temporal", "force"], "Invalid configuration!\n", "--residual cannot be combined with --temporal"),
    (["--gpus", "2"], "Invalid configuration!\n", "--residual cannot be combined with --gpus N > 1"),
    (["--pair-launch", "1"], "Invalid configuration!\n", "--residual cannot be combined with --pair-launch 1"),
])
def test_cli_residual_rejections(tmp_path, extra, stdout, reason):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + RES + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 255 and p.stdout == stdout, (p.returncode, p.stdout)
    assert reason in p.stderr, p.stderr
    assert not os.path.exists(out)
    p = _cli(["--3d", "--dtype", "fp32"] + extra + ["-o", out, stc], tmp_path)          # legal without the option
    assert p.returncode == 0, p.stdout + p.stderr


@pytest.mark.parametrize("value", ["l2", "min", ""])
def test_cli_residual_accepts_only_max(tmp_path, value):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32", "--residual", value, "-o", out, stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Illegal input.\n" and not os.path.exists(out), (p.returncode, p.stdout)


def test_slab_forms_refuse_residual(tmp_path):
    from drstencil_amd import multigpu
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    opts = ["--3d", "--dtype", "fp32"] + RES
    with pytest.raises(ValueError, match="--residual"):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match="--residual"):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match="--residual"):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match="--residual"):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    with pytest.raises(drs.KernelBuildError, match="--residual is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))


def test_bare_c4_residual_keeps_the_tuned_row():
    """--residual names the problem: a bare C4 command line still takes the tuner's row, and the kernel info's register demand grows by
    the centre stream's RY * VX * (PD + 1) words plus rmax."""
    args = ["--3d", "--dtype", "fp32"]
    rc0, msg0, src0 = drs.generate(args + [C4])
    rc1, msg1, src1 = drs.generate(args + RES + [C4])
    assert rc0 == rc1 == 0
    row = re.search(r"is used \((.*?)\)", msg0).group(1)
    assert "is used (%s)" % row in msg1
    i0, i1 = _info(src0), _info(src1)
    assert "cv1_0_0" in src1 and "cv2_0_0" not in src1 and "residual" not in i0
    assert i1["reg_demand"] == i0["reg_demand"] + i0["points_per_lane"] * 2 + 1
    # fp64: twice the words
    j0, j1 = (_info(drs.generate(["--3d", "--dtype", "fp64", "--sn", "8", "--prefetch"] + x + [rc.stc("t3_star")])[2]) for x in ([], RES))
    assert j1["reg_demand"] == j0["reg_demand"] + 2 * (j0["points_per_lane"] * 2 + 1)


def test_no_trace_without_residual():
    """A command line without --residual emits no trace of the option (the corpus of scripts/emit_corpus.py pins the whole text)."""
    seen = 0
    for cid, ndim, stc, opts in GPU_SMALL[::5] + [("c4", 3, C4, ["--3d", "--dtype", "fp32", "--step", "2"]), ("src", 3, rc.stc("t3_wave"), ["--3d", "--source", "--time-order", "2", "--store-mask", "buffer"])]:
        rc_, msg, src = drs.generate(opts + [stc])
        assert src is None or not any(w in src for w in ("pcen", "cv0_", "d_res", "residual", "rmax", "drs_wave_max", "_res(")), cid
        seen += src is not None
    assert seen >= 6


# ---- the C ABI's refusals (nothing is launched: the kernels are cross-compiled and loaded) ---------------------------------------------
def test_abi_refusals():
    cid, ndim, stc, opts = rc.EDGE[1]
    L = drs.lib()
    kres = drs.Kernel(rc.with_res(opts) + [stc])
    kplain = drs.Kernel(list(opts) + [stc])
    assert kres.residual_elems == kres.info["residual_elems"] == 1 + kres.info["grid"] and kplain.residual_elems == 0
    ms = __import__("ctypes").c_float()
    # an existing launch or run entry point on a --residual kernel
    assert L.drs_kernel_launch(kres.h, 1, 2, 0) == -2 and L.drs_kernel_run(kres.h, 1, 2, 4, 0, 0) == -2
    assert L.drs_kernel_run_timed(kres.h, 1, 2, 4, 0, 0, ms) == -2
    assert L.drs_kernel_launch_src(kres.h, 1, 2, 3, 0) == -2 and L.drs_kernel_run_src(kres.h, 1, 2, 3, 4, 0, 0) == -2
    # the new ones on a kernel without it
    assert L.drs_kernel_launch_res(kplain.h, 1, 2, None, 4, 0) == -2 and L.drs_kernel_run_res(kplain.h, 1, 2, None, 4, 4, 0) == -2
    assert L.drs_kernel_solve(kplain.h, 1, 2, None, 4, 1e-3, 8, 1, 0, None, None) == -2
    # a null d_res, and a source array on a kernel without --source
    assert L.drs_kernel_launch_res(kres.h, 1, 2, None, None, 0) == -2 and L.drs_kernel_run_res(kres.h, 1, 2, None, None, 4, 0) == -2
    assert L.drs_kernel_solve(kres.h, 1, 2, None, None, 1e-3, 8, 1, 0, None, None) == -2
    assert L.drs_kernel_launch_res(kres.h, 1, 2, 3, 4, 0) == -2
    for call in (kres.launch, kres.run, kres.run_timed):
        with pytest.raises(ValueError, match="d_res"):
            call(1, 2)
    for call in (kplain.launch, kplain.run, kplain.run_timed):
        with pytest.raises(ValueError, match="without --residual"):
            call(1, 2, d_res=3)
    with pytest.raises(ValueError):
        kplain.solve(1, 2, 3, 1e-3, 8)


# ---- emulated kernels against the host reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", rc.CASES, ids=[c[0] for c in rc.CASES])
def test_emulated_residual_cases(tmp_path, monkeypatch, cid, ndim, src, opts):
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    assert lib.info["residual"] == "max" and lib.info["stages"] == 1 and lib.residual_elems == 1 + lib.info["grid"]
    if cid == rc.BIG[0]:
        assert lib.info["stream_blocks"] == 9 and lib.info["tiles_x"] * lib.info["tiles_y"] == 18 and lib.info["grid"] == 168
    spec = oracle.Spec(stc, ndim, rc.step_of(opts))
    A0, B0, F0 = rc.inputs(spec, opts)
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _three_launches(lib, spec, ndim, opts, A0, B0, F0, (cid, "forward"))
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _three_launches(_second_lib(lib, tmp_path, "rev"), spec, ndim, opts, A0, B0, F0, (cid, "reverse"))
    # the gold kernel is the parent's: the same arrays, no residual
    A, B = A0.copy(), B0.copy()
    Ar, Br = A0.copy(), B0.copy()
    assert lib.gold(A, B, F0) == 0
    rc.host_launch(spec, ndim, opts, Ar, Br, F0)
    assert np.array_equal(A, Ar) and np.array_equal(B, Br)


_SAMPLE = list(enumerate(rc.sample_jobs()))
SMALL_GRID = {3: (13, 21, 300), 2: (1, 37, 300)}       # tiny ragged grids: more than one stream block, a partial x-edge tile


@pytest.mark.parametrize("n,job", _SAMPLE, ids=["%02d" % n for n, _ in _SAMPLE])
def test_emulated_residual_sampled_fuzz(tmp_path, monkeypatch, n, job):
    """The sample of the tuner's space on tiny grids.  What the generator refuses there it refuses with its own reason, and without
    --residual too unless the reason is the option's (on-chip stages)."""
    ndim, path, dtype, args, step = job
    opts = args[:-1]
    assert opts[-2:] == RES
    stc = _small_stc(tmp_path, path, ndim, SMALL_GRID[ndim])
    p = _cli(opts + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
    if p.returncode != 0:
        q = _cli(opts[:-2] + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
        assert p.returncode == 255 and ("--residual cannot be combined with --temporal" in p.stderr or q.returncode == 255), (p.stderr, q.stderr)
        return
    lib = rc.build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, step)
    A0, B0, F0 = rc.inputs(spec, opts)
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _three_launches(lib, spec, ndim, opts, A0, B0, F0, (n, "forward"))
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _three_launches(_second_lib(lib, tmp_path, "rev"), spec, ndim, opts, A0, B0, F0, (n, "reverse"))


def test_residual_sample_size():
    jobs = rc.sample_jobs()
    assert len(jobs) == rc.SAMPLE_SIZE == 20 and jobs == rc.sample_jobs() and all(j[3][-3:-1] == RES for j in jobs)


# ---- the planted maximum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", rc.PLANT, ids=[c[0] for c in rc.PLANT])
def test_emulated_planted_maximum(tmp_path, cid, ndim, src, opts):
    """in[p] = 1e3 at one interior cell per launch: the eight interior corners and both sides of a tile seam in x, in y and of a
    stream-block seam in z.  A lane or workgroup left out of the reduction reports the neighbours' roughly 200 instead of roughly 700."""
    stc = shutil.copy(src, str(tmp_path))
    lib = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0 = rc.inputs(spec, opts)
    cells = rc.planted_cells(lib.info)
    assert len(cells) >= (14 if cid == rc.BIG[0] else 10), (cid, len(cells))
    for cell in cells:
        A, B = A0.copy(), B0.copy()
        A[cell] = 1e3
        Ar, Br = A.copy(), B.copy()
        res = _nan_res(lib, A.dtype)
        assert lib.launch(A, B, F0, res) == 0
        want = rc.host_launch(spec, ndim, opts, Ar, Br, F0)
        assert 600 < want < 800 and rc.same_bits(res[0], want), (cid, cell, res[0], want)
        assert np.array_equal(B, Br)


# ---- poison -----------------------------------------------------------------------------------------------------------------------
_POISON = rc.PLANT + [rc.EDGE[5], rc.KNOBS[5], rc.MODES[2]]


@pytest.mark.parametrize("cid,ndim,src,opts", _POISON, ids=[c[0] for c in _POISON])
def test_emulated_poison(tmp_path, cid, ndim, src, opts):
    """NaN in every cell of `in` that neither a tap nor the centre stream reads, in out's ring and in src's ring, and in all of d_res
    before every launch: r is finite and exact and every element of d_res has been overwritten (a missing ownership predicate, an
    unwritten partial, a fold that reads a stale slot)."""
    from footprint import nan_value, ring_mask
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0 = rc.inputs(spec, opts)
    ring = ring_mask(spec.shape, spec.halo)
    A = rc.poisoned_input(A0, spec)
    B = B0.copy()
    B[ring] = nan_value(B.dtype)
    if F0 is not None:
        F0[ring] = nan_value(F0.dtype)
    Ar, Br = A.copy(), B.copy()
    for t in range(2):
        res = _nan_res(lib, A.dtype)
        assert lib.launch(A, B, F0, res) == 0
        want = rc.host_launch(spec, ndim, opts, Ar, Br, F0)
        assert np.isfinite(want) and rc.same_bits(res[0], want), (cid, t, res[0], want)
        assert not np.isnan(res).any(), (cid, t, np.argwhere(np.isnan(res))[:4])
        assert np.array_equal(rc.interior(B, spec.halo), rc.interior(Br, spec.halo)) and np.isnan(B[ring]).all()


# ---- special values -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", rc.PLANT, ids=[c[0] for c in rc.PLANT])
def test_emulated_special_values(tmp_path, cid, ndim, src, opts):
    stc = shutil.copy(src, str(tmp_path))
    lib = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    A0, B0, F0 = rc.inputs(spec, opts)
    mid = tuple(n // 2 for n in spec.shape)

    def one(A, B):
        Ar, Br = A.copy(), B.copy()
        res = _nan_res(lib, A.dtype)
        assert lib.launch(A, B, F0, res) == 0
        want = rc.host_launch(spec, ndim, opts, Ar, Br, F0)
        assert rc.same_bits(res[0], want), (cid, res[0], want)
        assert np.array_equal(np.isnan(B), np.isnan(Br))
        return res[0]

    # one NaN in an interior cell of in -> r is NaN; a second launch on finite data is finite: no state survives
    A = A0.copy()
    A[mid] = np.nan
    assert np.isnan(one(A, B0.copy()))
    assert np.isfinite(one(A0.copy(), B0.copy()))
    # +inf: out - in is inf - inf at the cell itself (the centre tap), +inf at its neighbours; numpy says NaN
    A = A0.copy()
    A[mid] = np.inf
    one(A, B0.copy())
    # -inf next to +inf, and a huge finite value whose difference overflows nothing
    A = A0.copy()
    A[mid] = np.inf
    A[mid[:-1] + (mid[-1] + 3,)] = -np.inf
    one(A, B0.copy())
    # an all-zero grid: +0.0 in bits (also with -0.0 cells: |(-0) - (-0)| = +0)
    Z = np.zeros_like(A0)
    r = one(Z.copy(), B0.copy())
    assert r.tobytes() == np.zeros((), A0.dtype).tobytes()
    Zm = Z.copy()
    Zm[tuple(slice(H, n - H) for n in Z.shape)] = -0.0
    r = one(Zm, B0.copy())
    assert r.tobytes() == np.zeros((), A0.dtype).tobytes()


# ---- unchanged arrays -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", rc.UNCHANGED, ids=[c[0] for c in rc.UNCHANGED])
def test_emulated_arrays_equal_those_without_the_option(tmp_path, cid, ndim, src, opts):
    stc = _case_stc(tmp_path, cid, ndim, src)
    with_opt = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    plain = rc.build_emulated(tmp_path, stc, list(opts))
    assert plain.residual_elems == 0 and "residual" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0 = rc.inputs(spec, opts)
    A1, B1, A2, B2 = A0.copy(), B0.copy(), A0.copy(), B0.copy()
    for t in range(2):
        res = _nan_res(with_opt, A0.dtype)
        a, b = ((A1, B1), (B1, A1))[t]
        assert with_opt.launch(a, b, F0, res) == 0
        a, b = ((A2, B2), (B2, A2))[t]
        assert plain.launch(a, b, F0) == 0
        assert np.array_equal(A1, A2) and np.array_equal(B1, B2), (cid, t)


# ---- memory contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", rc.CONTRACT, ids=[c[0] for c in rc.CONTRACT])
def test_residual_memory_contract(tmp_path, cid, ndim, src, opts):
    """in, out, src and a d_res of exactly residual_elems elements each flush against PROT_NONE pages (end-flush and start-flush), in a
    child process: no SIGSEGV, exact arrays and residual, every element of d_res written."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    job = {"so": lib.so, "stc": stc, "ndim": ndim, "opts": list(opts), "placements": ["end", "start"]}
    jpath = str(tmp_path / "job.json")
    with open(jpath, "w") as f:
        json.dump(job, f)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "residual_child.py"), jpath], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (p.returncode, p.stdout[-1500:], p.stderr[-1500:])


# ---- run to tolerance (the loop of drs_kernel_solve, driven here through the emulated plugin's launches) ----------------------------
def _emulated_solve(lib, A, B, F, tol, max_launches, check_every):
    """drs_kernel_solve's loop on an emulated plugin: the library's own loop needs a device; its decisions are these."""
    n, r = 0, None
    limit = max_launches - max_launches % 2
    res = _nan_res(lib, A.dtype)
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            assert lib.launch(A, B, F, res) == 0 and lib.launch(B, A, F, res) == 0
            n += 2
        r = res[0]
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r


def _solve_inputs(spec, dt, F_too):
    H = spec.halo
    A = np.zeros(spec.shape, dt)
    rc.interior(A, H)[...] = np.random.default_rng(21).random(tuple(n - 2 * H for n in spec.shape)).astype(dt)      # zero ring, random interior in [0, 1)
    F = None
    if F_too:
        F = np.zeros(spec.shape, dt)
        rc.interior(F, H)[...] = np.random.default_rng(22).random(tuple(n - 2 * H for n in spec.shape)).astype(dt) * 0.01
    return A, A.copy(), F


_SOLVE = rc.SOLVE + [rc.POISSON2]


@pytest.mark.parametrize("cid,ndim,src,opts,tol", _SOLVE, ids=[c[0] for c in _SOLVE])
def test_emulated_run_to_tolerance(tmp_path, cid, ndim, src, opts, tol):
    """jacobi3 (six neighbours at 1/6, no centre tap: the centre stream is the only reader of those cells) on 10^3 and the 2D Poisson
    case with --source on 12 x 12: the same launch count, residual bits and A as a numpy loop of oracle sweeps that looks at r at the
    same launches (check_every = 4 pairs)."""
    stc = rc.solve_stc(tmp_path, "emu", ndim, src)
    lib = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    spec = oracle.Spec(stc, ndim, 1)
    dt = rc.dtype_of(opts)
    A, B, F = _solve_inputs(spec, dt, "--source" in opts)
    Ar, Br = A.copy(), B.copy()
    want = rc.oracle_solve(spec, Ar, Br, F, tol, rc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and want[1] < rc.MAX_LAUNCHES // 2 and want[1] % 8 == 0, want
    got = _emulated_solve(lib, A, B, F, tol, rc.MAX_LAUNCHES, 4)
    print(cid, "launches", got[1], "residual", got[2])
    assert got[0] == 0 and got[1] == want[1] and rc.same_bits(got[2], want[2]), (got, want)
    assert np.array_equal(A, Ar)
    # max_launches = 16: status 1 with 16 launches
    A, B, F = _solve_inputs(spec, dt, "--source" in opts)
    assert _emulated_solve(lib, A, B, F, tol, 17, 4)[:2] == (1, 16)


def test_emulated_overflow_is_reported(tmp_path):
    """A centre cell of finfo.max under t3_star's coefficient sum of 1.5: inf within a few checks, status -4."""
    cid, ndim, src, opts = rc.DIVERGE
    stc = _small_stc(tmp_path, src, ndim, (13, 19, 140))
    lib = rc.build_emulated(tmp_path, stc, rc.with_res(opts))
    spec = oracle.Spec(stc, ndim, 1)
    A = np.ones(spec.shape, np.float32)
    A[tuple(n // 2 for n in spec.shape)] = np.finfo(np.float32).max
    with np.errstate(over="ignore", invalid="ignore"):
        status, n, r = _emulated_solve(lib, A, A.copy(), None, 1e-4, rc.MAX_LAUNCHES, 8)
    print("overflow reported after", n, "launches")
    assert status == -4 and n <= 10 * 16 and not np.isfinite(r), (status, n, r)
