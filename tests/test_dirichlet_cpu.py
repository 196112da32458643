"""--dirichlet (held cells inside the domain: out = fix where fix is not NaN) without a GPU: the generator's option surface, the C ABI's
refusals, and the emitted kernels under the CPU emulation (tests/emu) in both fiber orders -- whole arrays bit for bit against the job's
host reference followed by np.where on the interior, planted held cells at corners and seams and their complement, all free and all held,
NaN markers of every kind with held values arithmetic would not keep, the memory contract flush against inaccessible pages with a read
log over fix, the samples of the tuner's space, the residual of every mode and the run to tolerance around held cells.

The case list is tests/dirichlet_cases.py's, the one tests/test_dirichlet_gpu.py runs on the GPU.  The knob cases on t3_star run that
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

import dirichlet_cases as dc
import drstencil_amd as drs
import oracle
import residual_cases as rc
from emu_util import DRSTENCIL
from footprint import bit_equal
from gpu_cases import SMALL as GPU_SMALL
from helpers import write_stc
from special_values import count_different, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = os.path.join(ROOT, "benchmarks", "configs", "c4_3d7pt_star_1024.stc")
DIR = dc.DIR
# grids of the emulated knob cases: (L, M, N)
DIMS = {"prefetch_depth2": (19, 37, 264), "defer_stores": (13, 19, 264), "rows_pack": (21, 19, 264), "cyclic_merge_x2_fp64": (13, 19, 140),
        "loader_waves_fp64": (13, 19, 140), "store_mask_buffer": (13, 37, 264), "odd_elem_fp64": (13, 21, 135), "tile_2d_fp32": (1, 41, 268),
        "tile_2d_box9_fp64": (1, 41, 140), "stream_2d_fp32": (1, 61, 268), "stream_2d_dma_fp64": (1, 45, 140)}


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
    return dc.load_emulated(cp)


def _nan_res(lib, dt):
    return np.full(lib.residual_elems, np.nan, dt) if lib.residual_elems else None


def _launches(lib, spec, ndim, opts, A0, B0, F0, X, what, launches=3, gold=False):
    """`launches` launches from (A0, B0, F0) with held cells X: after each, both WHOLE arrays equal the host reference's in bits; with
    --residual max r equals numpy's in bits and every element of the NaN-filled residual array has been overwritten."""
    A, B = A0.copy(), B0.copy()
    Ar, Br = A0.copy(), B0.copy()
    X0, F00 = X.copy(), None if F0 is None else F0.copy()
    for t in range(launches):
        s, d = (A, B) if t % 2 == 0 else (B, A)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        res = None if gold else _nan_res(lib, A.dtype)
        assert (lib.gold(s, d, F0, X) if gold else lib.launch(s, d, F0, res, X)) == 0
        want = dc.host_launch(spec, ndim, opts, sr, dr, F0, X)
        assert same_bits(A, Ar) and same_bits(B, Br), (what, t, count_different(A, Ar), count_different(B, Br))
        if res is not None:
            assert rc.same_bits(res[0], want), (what, t, res[0], want)
            assert not np.isnan(res).any() or np.isnan(want), (what, t, "partials not written")
    assert bit_equal(X, X0) and (F0 is None or bit_equal(F0, F00)), (what, "fix or src was written")
    return A, B


def _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, opts, A0, B0, F0, X, what, launches=3, tag="rev"):
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, (what, "forward"), launches)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, (what, "gold"), launches, gold=True)
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _launches(_second_lib(lib, tmp_path, tag), spec, ndim, opts, A0, B0, F0, X, (what, "reverse"), launches)      # (a loaded copy is never overwritten: one tag per call)


# ---- 8. interface: generator / CLI --------------------------------------------------------------------------------------------------
def test_cli_dirichlet(tmp_path):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (10, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + DIR + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "held" not in p.stdout and "dirichlet" not in p.stdout              # stdout stays the reference's protocol
    notes = [ln for ln in p.stderr.splitlines() if "held cells" in ln]
    assert len(notes) == 1 and notes[0].startswith("drstencil: note: held cells: a launch takes one more array fix")
    src = open(out).read()
    info = _info(src)
    assert info["dirichlet"] == 1 and "source" not in info and "residual" not in info
    assert re.search(r"^// options: --3d --dtype fp32 -o \S+ --dirichlet$", src, re.M)
    assert "const real_t* __restrict__ d_in, real_t* __restrict__ d_out, const real_t* __restrict__ d_fix)" in src
    assert "drs_plugin_launch_fix(const void* in, void* out, const void* src, void* res, const void* fix, hipStream_t stream)" in src
    assert "drs_plugin_launch_gold_fix(const void* in, void* out, const void* src, const void* fix, hipStream_t stream)" in src
    assert not any(n + "(" in src for n in dc.Emulated.OTHERS)
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert "d_out[((long)k * M + j) * N + i] = (f != f) ? t : f;" in gold
    rc2, msg, src2 = drs.generate(["--3d", "--dtype", "fp32"] + DIR + ["-o", out, stc])
    assert rc2 == 0 and src2 == src and "drstencil: note: held cells:" in msg
    # the option has one place in the banner wherever it stands: the same command, the same text
    rc3, msg3, src3 = drs.generate(["--dirichlet", "--3d", "--dirichlet", "--dtype", "fp32", "-o", out, stc])
    assert rc3 == 0 and src3 == src
    # with every other array: in, out, src, res, fix; gold without res; the select behind - out_old and + src
    p = _cli(["--3d", "--dtype", "fp32", "--source", "--time-order", "2", "--residual", "max"] + DIR + ["-o", out, stc], tmp_path)
    src = open(out).read()
    assert p.returncode == 0 and "real_t* __restrict__ d_out, const real_t* __restrict__ d_src, real_t* __restrict__ d_res, const real_t* __restrict__ d_fix)" in src
    assert "(const real_t*)in, (real_t*)out, (const real_t*)src, (real_t*)res, (const real_t*)fix);" in src and "res_p, dim3(1)" in src
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert gold.index("t = t - d_out[") < gold.index("t = t + d_src[") < gold.index("(f != f) ? t : f") and "d_res" not in gold
    info = _info(src)
    assert info["dirichlet"] == 1 and info["source"] == 1 and info["time_order"] == 2 and info["residual"] == "max"
    assert not any(n + "(" in src for n in dc.Emulated.OTHERS)
    assert "--dirichlet " in drs.generate(["--help"])[1]


@pytest.mark.parametrize("extra,reason", [
    (["--step", "2"], "--dirichlet needs --step 1 (a fused S^n through held cells is not n held steps)"),
    (["--step", "2", "--temporal", "1"], "--dirichlet needs --step 1"),
    (["--temporal", "force"], "--dirichlet cannot be combined with --temporal"),
    (["--gpus", "2"], "--dirichlet cannot be combined with --gpus N > 1"),
    (["--pair-launch", "1"], "--dirichlet cannot be combined with --pair-launch 1"),
])
def test_cli_dirichlet_rejections(tmp_path, extra, reason):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + DIR + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", (p.returncode, p.stdout)
    assert reason in p.stderr, p.stderr
    assert not os.path.exists(out)
    p = _cli(["--3d", "--dtype", "fp32"] + extra + ["-o", out, stc], tmp_path)          # legal without the option
    assert p.returncode == 0, p.stdout + p.stderr


def test_slab_forms_refuse_dirichlet(tmp_path):
    from drstencil_amd import multigpu
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    opts = ["--3d", "--dtype", "fp32"] + DIR
    with pytest.raises(ValueError, match="--dirichlet"):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match="--dirichlet"):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match="--dirichlet"):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match="--dirichlet"):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    with pytest.raises(drs.KernelBuildError, match="--dirichlet is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))


def test_bare_c4_dirichlet_keeps_the_tuned_row():
    """--dirichlet names the problem: a bare C4 command line still takes the tuner's step-1 row, and the kernel info's register demand
    grows by the fix stream's RY * VX * (PD + 1) words (twice that in fp64)."""
    args = ["--3d", "--dtype", "fp32"]
    rc0, msg0, src0 = drs.generate(args + ["--step", "1", C4])
    rc1, msg1, src1 = drs.generate(args + DIR + [C4])
    assert rc0 == rc1 == 0
    row = re.search(r"is used \((.*?)\)", msg0).group(1)
    assert "is used (%s)" % row in msg1
    i0, i1 = _info(src0), _info(src1)
    assert "fv1_0_0" in src1 and "fv2_0_0" not in src1 and "dirichlet" not in i0
    assert i1["reg_demand"] == i0["reg_demand"] + i0["points_per_lane"] * 2
    j0, j1 = (_info(drs.generate(["--3d", "--dtype", "fp64", "--sn", "8", "--prefetch"] + x + [rc.stc("t3_star")])[2]) for x in ([], DIR))
    assert j1["reg_demand"] == j0["reg_demand"] + 2 * j0["points_per_lane"] * 2


def test_no_trace_without_dirichlet():
    """A command line without --dirichlet emits no trace of the option (the corpus of scripts/emit_corpus.py pins the whole text)."""
    seen = 0
    older = GPU_SMALL[::5] + [("c4", 3, C4, ["--3d", "--dtype", "fp32", "--step", "2"]),
                              ("src", 3, rc.stc("t3_wave"), ["--3d", "--source", "--time-order", "2", "--store-mask", "buffer", "--residual", "max"])]
    for cid, ndim, stc, opts in older:
        rc_, msg, src = drs.generate(opts + [stc])
        assert src is None or not any(w in src for w in ("pfix", "fv0_", "d_fix", "dirichlet", "held cells", "_fix(")), cid
        seen += src is not None
        if src is not None and "--step" not in opts:
            rc_, msg, src = drs.generate(opts + DIR + [stc])
            assert rc_ == 0 and "pfix" in src and _info(src)["dirichlet"] == 1, cid
    assert seen >= 6


# ---- 8. the C ABI's refusals (nothing is launched: the kernels are cross-compiled and loaded) -----------------------------------------
def test_abi_refusals():
    import ctypes
    cid, ndim, stc, opts = dc.EDGE[1]
    L = drs.lib()
    kfix = drs.Kernel(dc.with_fix(opts) + [stc])
    kplain = drs.Kernel(list(opts) + [stc])
    assert kfix.dirichlet and kfix.info["dirichlet"] == 1 and not kplain.dirichlet and "dirichlet" not in kplain.info
    assert kfix.bytes_per_launch() == kplain.bytes_per_launch() * 3 // 2
    ms = ctypes.c_float()
    # every existing launch or run entry point on a --dirichlet kernel
    assert L.drs_kernel_launch(kfix.h, 1, 2, 0) == -2 and L.drs_kernel_launch_gold(kfix.h, 1, 2, 0) == -2
    assert L.drs_kernel_run(kfix.h, 1, 2, 4, 0, 0) == -2 and L.drs_kernel_run_timed(kfix.h, 1, 2, 4, 0, 0, ms) == -2
    assert L.drs_kernel_launch_src(kfix.h, 1, 2, 3, 0) == -2 and L.drs_kernel_launch_gold_src(kfix.h, 1, 2, 3, 0) == -2
    assert L.drs_kernel_run_src(kfix.h, 1, 2, 3, 4, 0, 0) == -2 and L.drs_kernel_run_timed_src(kfix.h, 1, 2, 3, 4, 0, 0, ms) == -2
    assert L.drs_kernel_launch_res(kfix.h, 1, 2, None, 4, 0) == -2 and L.drs_kernel_run_res(kfix.h, 1, 2, None, 4, 4, 0) == -2
    assert L.drs_kernel_solve(kfix.h, 1, 2, None, 4, 1e-3, 8, 1, 0, None, None) == -2
    # the new ones on a kernel without the option
    assert L.drs_kernel_launch_fix(kplain.h, 1, 2, None, None, 5, 0) == -2 and L.drs_kernel_launch_gold_fix(kplain.h, 1, 2, None, 5, 0) == -2
    assert L.drs_kernel_run_fix(kplain.h, 1, 2, None, None, 5, 4, 0, 0) == -2 and L.drs_kernel_run_timed_fix(kplain.h, 1, 2, None, None, 5, 4, 0, 0, ms) == -2
    assert L.drs_kernel_solve_fix(kplain.h, 1, 2, None, 4, 5, 1e-3, 8, 1, 0, None, None) == -2
    # a null d_fix; a source or residual array on a kernel without those options; solve without --residual max
    assert L.drs_kernel_launch_fix(kfix.h, 1, 2, None, None, None, 0) == -2 and L.drs_kernel_launch_gold_fix(kfix.h, 1, 2, None, None, 0) == -2
    assert L.drs_kernel_launch_fix(kfix.h, 1, 2, 3, None, 5, 0) == -2 and L.drs_kernel_launch_fix(kfix.h, 1, 2, None, 4, 5, 0) == -2
    assert L.drs_kernel_launch_gold_fix(kfix.h, 1, 2, 3, 5, 0) == -2
    assert L.drs_kernel_solve_fix(kfix.h, 1, 2, None, None, 5, 1e-3, 8, 1, 0, None, None) == -2
    for call in (kfix.launch, kfix.launch_gold, kfix.run, kfix.run_timed):
        with pytest.raises(ValueError, match="needs d_fix"):
            call(1, 2)
    for call in (kplain.launch, kplain.launch_gold, kplain.run, kplain.run_timed):
        with pytest.raises(ValueError, match="without --dirichlet"):
            call(1, 2, d_fix=3)
    with pytest.raises(ValueError):
        kfix.solve(1, 2, None, 1e-3, 8, d_fix=5)
    with pytest.raises(ValueError, match="without --dirichlet"):
        kplain.solve(1, 2, None, 1e-3, 8, d_fix=5)


# ---- 1. bit-exactness -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_emulated_dirichlet_cases(tmp_path, monkeypatch, cid, ndim, src, opts):
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = dc.build_emulated(tmp_path, stc, dc.with_fix(opts))
    assert lib.info["dirichlet"] == 1 and lib.info["stages"] == 1
    if cid == dc.BIG[0]:
        assert lib.info["stream_blocks"] == 9 and lib.info["tiles_x"] * lib.info["tiles_y"] == 18 and lib.info["grid"] == 168
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X = dc.inputs(spec, opts)
    if cid == dc.MIN_333[0]:
        # one interior cell: once held, once free
        for v in (0.375, np.nan):
            X[1, 1, 1] = v
            _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, opts, A0, B0, F0, X, (cid, v), tag="rev_%s" % ("free" if np.isnan(v) else "held"))
        return
    held, free = dc.held_and_free(X, spec.halo)
    assert held >= 1 and free >= 1, (cid, held, free)                      # on the pattern alone
    _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, opts, A0, B0, F0, X, cid)


# ---- 2. planted cells -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", dc.PLANT, ids=[c[0] for c in dc.PLANT])
def test_emulated_planted_cells(tmp_path, cid, ndim, src, opts):
    """Held: exactly the interior corners and both sides of every x, y and z seam; then exactly their complement."""
    stc = shutil.copy(src, str(tmp_path))
    lib = dc.build_emulated(tmp_path, stc, dc.with_fix(opts))
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, _ = dc.inputs(spec, opts)
    cells = rc.planted_cells(lib.info)
    assert len(cells) >= (14 if cid.startswith(dc.BIG[0]) else 10), (cid, len(cells))
    vals = dc.fix_pattern(spec.shape, A0.dtype, 5)
    vals[np.isnan(vals)] = 0.625
    planted = np.zeros(spec.shape, bool)
    for c in cells:
        planted[c] = True
    for mask in (planted, ~planted):
        X = np.where(mask, vals, np.asarray(np.nan, A0.dtype)).astype(A0.dtype)
        A, B = _launches(lib, spec, ndim, opts, A0, B0, F0, X, (cid, int(mask.sum())), launches=2)
        I = tuple(slice(spec.halo, n - spec.halo) for n in spec.shape)
        assert np.array_equal(B[I][mask[I]], vals[I][mask[I]]) and not np.array_equal(B[I][~mask[I]], vals[I][~mask[I]])


# ---- 3. all free, all held ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", dc.UNCHANGED, ids=[c[0] for c in dc.UNCHANGED])
def test_emulated_all_free_equals_the_plain_command(tmp_path, cid, ndim, src, opts):
    stc = _case_stc(tmp_path, cid, ndim, src)
    with_opt = dc.build_emulated(tmp_path, stc, dc.with_fix(opts))
    plain = dc.build_emulated(tmp_path, stc, list(opts))
    assert not plain.dirichlet and "dirichlet" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X = dc.inputs(spec, opts)
    X[...] = np.nan
    A1, B1, A2, B2 = A0.copy(), B0.copy(), A0.copy(), B0.copy()
    for t in range(2):
        a, b = ((A1, B1), (B1, A1))[t]
        assert with_opt.launch(a, b, F0, None, X) == 0
        a, b = ((A2, B2), (B2, A2))[t]
        assert plain.launch(a, b, F0) == 0
        assert bit_equal(A1, A2) and bit_equal(B1, B2), (cid, t)


@pytest.mark.parametrize("cid,ndim,src,opts", dc.UNCHANGED, ids=[c[0] for c in dc.UNCHANGED])
def test_emulated_all_held(tmp_path, cid, ndim, src, opts):
    """fix NaN-free, `in` entirely NaN: the output's interior is fix's interior, its ring and all of `in` are bit-unchanged."""
    from footprint import nan_filled
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = dc.build_emulated(tmp_path, stc, dc.with_fix(opts))
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    A0, B0, F0, _ = dc.inputs(spec, opts)
    X = rc.inputs(spec, opts, 31)[0]                                  # NaN-free: every cell held
    A = nan_filled(spec.shape, A0.dtype)
    assert "--boundary" not in opts                                   # (a ring fill would rewrite in's ring)
    Ain, B = A.copy(), B0.copy()
    assert lib.launch(A, B, F0, None, X) == 0
    assert bit_equal(A, Ain)
    want = B0.copy()
    rc.interior(want, H)[...] = rc.interior(X, H)
    assert bit_equal(B, want), (cid, count_different(B, want))


# ---- 4. sentinels and special values --------------------------------------------------------------------------------------------------
def _special_reference(spec, ndim, opts, A, B, F, X, cells):
    """The reference of one launch, and the four built conditions asserted on it alone."""
    Ar, Br = A.copy(), B.copy()
    unheld = np.zeros_like(A)
    dc.host_launch(spec, ndim, opts, Ar, Br, F, X, unheld=unheld)
    m0 = np.asarray(-0.0, A.dtype).tobytes()
    assert not np.isnan(X[cells["held_nan"]]) and np.isnan(unheld[cells["held_nan"]])               # a held cell whose unheld value is NaN
    assert not np.isnan(X[cells["held_inf"]]) and np.isinf(unheld[cells["held_inf"]])               # ... is inf
    assert np.isnan(X[cells["free_nan"]]) and np.isnan(Br[cells["free_nan"]])                       # a free cell whose value is NaN
    assert np.isnan(X[cells["free_m0"]]) and Br[cells["free_m0"]].tobytes() == m0                   # a free cell whose value is -0.0
    assert Br[cells["held_nan"]] == 0.5 and Br[cells["held_inf"]] == -0.25
    return Ar, Br


@pytest.mark.parametrize("cid,ndim,src,opts", dc.PLANT, ids=[c[0] for c in dc.PLANT])
def test_emulated_special_values(tmp_path, cid, ndim, src, opts):
    """Free cells marked by NaNs of both signs, quiet and signalling, with payloads; held values +0.0, -0.0, the smallest subnormals and
    +-inf; NaN, inf and -0.0 planted in `in` so that a select and a blend m * v + (1 - m) * fix differ.  (The blend, tried once by hand in
    emit_fix_select and in the gold kernel, passes test_emulated_dirichlet_cases and fails here.)"""
    stc = shutil.copy(src, str(tmp_path))
    lib = dc.build_emulated(tmp_path, stc, dc.with_fix(opts))
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, cells = dc.special_problem(spec, opts)
    xi = rc.interior(X, spec.halo)
    seen = set(xi[np.isnan(xi)].view(dc._UINT[xi.dtype]).tolist())
    assert seen >= set(dc.FREE_NANS[np.dtype(xi.dtype)])
    for v in dc.held_specials(xi.dtype):
        assert (xi.view(dc._UINT[xi.dtype]) == np.asarray(v).view(dc._UINT[xi.dtype])).any(), v
    Ar, Br = _special_reference(spec, ndim, opts, A0, B0, F0, X, cells)
    for gold in (False, True):
        A, B = A0.copy(), B0.copy()
        assert (lib.gold(A, B, F0, X) if gold else lib.launch(A, B, F0, None, X)) == 0
        assert same_bits(A, Ar) and same_bits(B, Br), (cid, gold, count_different(B, Br))
        # the second launch carries the held infinities and the NaNs through the sweep
        Ar2, Br2 = Ar.copy(), Br.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            dc.host_launch(spec, ndim, opts, Br2, Ar2, F0, X)
        assert (lib.gold(B, A, F0, X) if gold else lib.launch(B, A, F0, None, X)) == 0
        assert same_bits(A, Ar2) and same_bits(B, Br2), (cid, gold, count_different(A, Ar2))


# ---- 5. memory contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", dc.CONTRACT, ids=[c[0] for c in dc.CONTRACT])
def test_dirichlet_memory_contract(tmp_path, cid, ndim, src, opts):
    """in, out, src, fix (and d_res) each flush against PROT_NONE pages (end-flush and start-flush), in a child process: no SIGSEGV, exact
    arrays, out's ring unchanged, fix unwritten and its NaN-free garbage ring without effect."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    for o in (list(opts), list(opts) + rc.RES):
        lib = dc.build_emulated(tmp_path, stc, dc.with_fix(o))
        job = {"so": lib.so, "stc": stc, "ndim": ndim, "opts": dc.with_fix(o), "placements": ["end", "start"]}
        jpath = str(tmp_path / "job.json")
        with open(jpath, "w") as f:
            json.dump(job, f)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dirichlet_child.py"), jpath], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (o, p.returncode, p.stdout[-1500:], p.stderr[-1500:])


@pytest.mark.parametrize("cid,ndim,src,opts", dc.READLOG, ids=[c[0] for c in dc.READLOG])
def test_fix_read_log(tmp_path, cid, ndim, src, opts):
    """With tests/source_readlog.h in front and the watch laid over fix, one launch reads every interior byte of fix and no ring byte."""
    from footprint import ring_mask
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = dc.build_emulated(tmp_path, stc, dc.with_fix(opts), read_log=True)
    spec = oracle.Spec(stc, ndim, 1)
    A, B, F, X = dc.inputs(spec, opts)
    seen = np.zeros(X.nbytes, np.uint8)
    lib.lib.drs_readlog_watch(X.ctypes.data, X.nbytes, seen.ctypes.data)
    assert lib.launch(A, B, F, None, X) == 0
    lib.lib.drs_readlog_watch(None, 0, None)
    seen = seen.reshape(spec.shape + (X.itemsize,))
    ring = ring_mask(spec.shape, spec.halo)
    assert seen[~ring].all(), (cid, "interior bytes of fix not read", int((seen[~ring] == 0).sum()))
    assert not seen[ring].any(), (cid, "ring bytes of fix read", int(seen[ring].sum()))


# ---- 6. the samples of the tuner's space ----------------------------------------------------------------------------------------------
SMALL_GRID = {3: (13, 21, 300), 2: (1, 37, 300)}       # tiny ragged grids: more than one stream block, a partial x-edge tile
_SAMPLE = [(w, n, j) for w in dc.SAMPLES for n, j in enumerate(dc.sample_jobs(w))]


@pytest.mark.parametrize("which,n,job", _SAMPLE, ids=["%s-%02d" % (w, n) for w, n, _ in _SAMPLE])
def test_emulated_dirichlet_sampled_fuzz(tmp_path, monkeypatch, which, n, job):
    """The samples on tiny grids.  What the generator refuses there it refuses without --dirichlet too, for its own reason."""
    ndim, path, dtype, args, step = job
    opts = args[:-1]
    assert "--dirichlet" in opts and step == 1
    stc = _small_stc(tmp_path, path, ndim, SMALL_GRID[ndim])
    p = _cli(opts + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
    if p.returncode != 0:
        q = _cli(dc.plain_opts(opts) + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
        assert p.returncode == 255 and q.returncode == 255 and "--dirichlet" not in p.stderr, (p.stderr, q.stderr)
        return
    lib = dc.build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, step)
    A0, B0, F0, X = dc.inputs(spec, opts)
    held, free = dc.held_and_free(X, spec.halo)
    assert held >= 1 and free >= 1
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, (which, n, "forward"))
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _launches(_second_lib(lib, tmp_path, "rev"), spec, ndim, opts, A0, B0, F0, X, (which, n, "reverse"))


def test_dirichlet_sample_size():
    for w in dc.SAMPLES:
        jobs = dc.sample_jobs(w)
        assert len(jobs) == dc.SAMPLE_SIZE == 20 and jobs == dc.sample_jobs(w) and all(j[3][-2] == "--dirichlet" for j in jobs)
        assert all(("--source" in j[3] and "--time-order" in j[3]) == (w != "dirichlet") for j in jobs)


# ---- 7. residual and run to tolerance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", dc.RES_MODES, ids=[c[0] for c in dc.RES_MODES])
def test_emulated_residual_with_held_cells(tmp_path, monkeypatch, cid, ndim, src, opts):
    """r = np.max(np.abs(out_I - in_I)) in bits after every launch, held cells included (the update sits behind the select)."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = dc.build_emulated(tmp_path, stc, dc.with_fix(opts))
    assert lib.residual_elems == 1 + lib.info["grid"] and lib.dirichlet
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X = dc.inputs(spec, opts)
    _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, opts, A0, B0, F0, X, cid)
    # once `in` holds the held values they contribute +0.0: hold everything, r is +0.0 in bits from the second launch on
    Xall = rc.inputs(spec, opts, 31)[0]
    A, B = A0.copy(), B0.copy()
    for s, d in ((A, B), (B, A)):
        res = _nan_res(lib, A.dtype)
        assert lib.launch(s, d, F0, res, Xall) == 0
    assert res[0].tobytes() == np.zeros((), A.dtype).tobytes()


def _emulated_solve(lib, A, B, F, X, tol, max_launches, check_every):
    """drs_kernel_solve_fix's loop on an emulated plugin: the library's own loop needs a device; its decisions are these."""
    n, r = 0, None
    limit = max_launches - max_launches % 2
    res = _nan_res(lib, A.dtype)
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            assert lib.launch(A, B, F, res, X) == 0 and lib.launch(B, A, F, res, X) == 0
            n += 2
        r = res[0]
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r


_SOLVE = [(c[0] + "_" + k, c[1], c[2], c[3], c[4], k) for c in dc.SOLVE for k in dc.SOLVE_KINDS]


@pytest.mark.parametrize("cid,ndim,src,opts,tol,kind", _SOLVE, ids=[c[0] for c in _SOLVE])
def test_emulated_run_to_tolerance(tmp_path, cid, ndim, src, opts, tol, kind):
    """jacobi3 on 10^3 with a ring of 0: an inner block held at 1.0, and an octant held at 0 (an L-shaped domain).  Status, launch count and
    r equal a numpy loop of oracle sweeps with the np.where after each, looking at r at the same launches (check_every = 4 pairs); held cells
    are bit-exactly their values in A and B; every value lies in [0, 1] (the maximum principle)."""
    stc = rc.solve_stc(tmp_path, "emu", ndim, src)
    o = opts + rc.RES
    lib = dc.build_emulated(tmp_path, stc, dc.with_fix(o))
    spec = oracle.Spec(stc, ndim, 1)
    dt = dc.dtype_of(opts)
    A, B, X = dc.solve_problem(spec, dt, kind)
    Ar, Br = A.copy(), B.copy()
    want = dc.oracle_solve(spec, Ar, Br, None, X, tol, dc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and want[1] < dc.MAX_LAUNCHES and want[1] % 8 == 0, want
    got = _emulated_solve(lib, A, B, None, X, tol, dc.MAX_LAUNCHES, 4)
    print(cid, "launches", got[1], "residual", got[2])
    assert got[0] == 0 and got[1] == want[1] and rc.same_bits(got[2], want[2]), (got, want)
    assert bit_equal(A, Ar) and bit_equal(B, Br)
    held = ~np.isnan(X)
    assert bit_equal(A[held], X[held]) and bit_equal(B[held], X[held])
    assert A.min() >= 0.0 and A.max() <= 1.0 and B.min() >= 0.0 and B.max() <= 1.0
    if kind == "block":
        assert A[~held].max() > 0.1                                    # the electrode's potential has spread
    # max_launches = 16: status 1 with 16 launches
    A, B, X = dc.solve_problem(spec, dt, kind)
    assert _emulated_solve(lib, A, B, None, X, tol, 17, 4)[:2] == (1, 16)
