"""--scale (a per-cell factor: out = c*in + w*S(in)) without a GPU: the generator's option surface, the C ABI's refusals, and the emitted
kernels under the CPU emulation (tests/emu) in both fiber orders -- whole arrays bit for bit against the host reference of
tests/scale_cases.py, unit scale against the same command without the option, the frozen field, planted factors at corners and seams and
their complement, the contracted variants the kernel must not compute, IEEE special values in w, the memory contract flush against
inaccessible pages with a read log over w, the samples of the tuner's space and the run to tolerance on screened Poisson.

The case list is tests/scale_cases.py's, the one tests/test_scale_gpu.py runs on the GPU.  The knob cases on t3_star run that stencil on
smaller grids here (more than one tile and stream block, partial tiles), so that each takes seconds under the emulation; the 70 x 45 x 530
case with early-leaving workgroups keeps its size."""
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
import scale_cases as sc
from emu_util import DRSTENCIL
from footprint import bit_equal, ring_mask
from gpu_cases import SMALL as GPU_SMALL
from helpers import write_stc
from special_values import count_different, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = os.path.join(ROOT, "benchmarks", "configs", "c4_3d7pt_star_1024.stc")
SCALE = sc.SCALE
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


def _geom(cid):
    """The geometry's id of a case id (the case list appends the centre or the mode's variant)."""
    return next((k for k in DIMS if cid.startswith(k)), None)


def _case_stc(tmp_path, cid, ndim, src):
    g = _geom(cid)
    return _small_stc(tmp_path, src, ndim, DIMS[g]) if g else shutil.copy(src, str(tmp_path))


def _info(src):
    return json.loads(re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', src).group(1).replace('\\"', '"'))


def _second_lib(lib, tmp_path, tag):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    cp = os.path.join(str(tmp_path), tag + "_" + os.path.basename(lib.so))
    shutil.copy(lib.so, cp)
    return sc.load_emulated(cp)


def _nan_res(lib, dt):
    return np.full(lib.residual_elems, np.nan, dt) if lib.residual_elems else None


def _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, what, launches=3, gold=False):
    """`launches` launches from (A0, B0) with src F0, held cells X and factors W: after each, both WHOLE arrays equal the host reference's
    in bits; with --residual max r equals numpy's in bits and every element of the NaN-filled residual array has been overwritten.
    Afterwards w, src and fix are bit-unchanged."""
    A, B = A0.copy(), B0.copy()
    Ar, Br = A0.copy(), B0.copy()
    keep = [None if a is None else a.copy() for a in (F0, X, W)]
    for t in range(launches):
        s, d = (A, B) if t % 2 == 0 else (B, A)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        res = None if gold else _nan_res(lib, A.dtype)
        assert (lib.gold(s, d, F0, X, W) if gold else lib.launch(s, d, F0, res, X, W)) == 0
        want = sc.host_launch(spec, ndim, opts, sr, dr, F0, X, W)
        assert same_bits(A, Ar) and same_bits(B, Br), (what, t, count_different(A, Ar), count_different(B, Br))
        if res is not None:
            assert rc.same_bits(res[0], want), (what, t, res[0], want)
            assert not np.isnan(res).any() or np.isnan(want), (what, t, "partials not written")
    for a, k in zip((F0, X, W), keep):
        assert a is None or bit_equal(a, k), (what, "src, fix or w was written")
    return A, B


def _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, opts, A0, B0, F0, X, W, what, launches=3, tag="rev"):
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, (what, "forward"), launches)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, (what, "gold"), launches, gold=True)
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _launches(_second_lib(lib, tmp_path, tag), spec, ndim, opts, A0, B0, F0, X, W, (what, "reverse"), launches)      # (a loaded copy is never overwritten: one tag per call)


# ---- 10. interface: generator / CLI -------------------------------------------------------------------------------------------------
def test_cli_scale(tmp_path):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (10, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + SCALE + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "scale" not in p.stdout and "factor" not in p.stdout                # stdout stays the reference's protocol
    notes = [ln for ln in p.stderr.splitlines() if "per-cell factor" in ln]
    assert len(notes) == 1 and notes[0].startswith("drstencil: note: per-cell factor: a launch takes one more array w and computes w * S(in)")
    src = open(out).read()
    info = _info(src)
    assert info["scale"] == 1 and info["scale_centre"] == 0 and "source" not in info and "residual" not in info and "dirichlet" not in info
    assert re.search(r"^// options: --3d --dtype fp32 -o \S+ --scale$", src, re.M)
    assert "const real_t* __restrict__ d_in, real_t* __restrict__ d_out, const real_t* __restrict__ d_scale)" in src
    assert "drs_plugin_launch_ops(const void* in, void* out, const void* src, void* res, const void* fix, const void* scale, hipStream_t stream)" in src
    assert "drs_plugin_launch_gold_ops(const void* in, void* out, const void* src, const void* fix, const void* scale, hipStream_t stream)" in src
    assert not any(n + "(" in src for n in sc.Emulated.OTHERS)
    # no centre term: the centre stream is not loaded
    assert "pcen" not in src and "cv0_" not in src and "const real_t t = " not in src
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert "t = d_scale[((long)k * M + j) * N + i] * t;" in gold and "c[0]; t = u + t" not in gold
    rc2, msg, src2 = drs.generate(["--3d", "--dtype", "fp32"] + SCALE + ["-o", out, stc])
    assert rc2 == 0 and src2 == src and "drstencil: note: per-cell factor:" in msg
    # the options have one place in the banner wherever they stand; --scale-centre 0 is the default spelled out
    rc3, msg3, src3 = drs.generate(["--scale", "--3d", "--scale", "--scale-centre", "0", "--dtype", "fp32", "-o", out, stc])
    assert rc3 == 0 and src3 == src
    # the centre term: the coefficient as a coefficient is written, two statements, one centre stream
    p = _cli(["--scale-centre", "0.30000001", "--3d", "--scale", "--dtype", "fp32", "-o", out, stc], tmp_path)
    src = open(out).read()
    assert p.returncode == 0 and re.search(r"^// options: --3d --dtype fp32 -o \S+ --scale --scale-centre 0.3$", src, re.M)
    assert _info(src)["scale_centre"] == 0.3 and "(0.3) * in + w * S(in)" in p.stderr
    assert "{ const real_t t = (real_t)(0.3) * cv0_0_0" in src and "pcen += DRS_STRIDE_S;" in src and "pscl += DRS_STRIDE_S;" in src and "rmax" not in src
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert gold.index("t = d_scale[") < gold.index("{ const real_t u = (real_t)(0.3) * c[0]; t = u + t; }")
    # with every other array: in, out, src, res, fix, w; gold without res; w first, the centre term, - out_old, + src, the select
    p = _cli(["--3d", "--dtype", "fp32", "--source", "--time-order", "2", "--residual", "max", "--dirichlet"] + SCALE + ["--scale-centre", "2", "-o", out, stc], tmp_path)
    src = open(out).read()
    assert p.returncode == 0 and ("real_t* __restrict__ d_out, const real_t* __restrict__ d_src, real_t* __restrict__ d_res, const real_t* __restrict__ d_fix, "
                                  "const real_t* __restrict__ d_scale)") in src
    assert "(const real_t*)in, (real_t*)out, (const real_t*)src, (real_t*)res, (const real_t*)fix, (const real_t*)scale);" in src and "res_p, dim3(1)" in src
    assert re.search(r"--dirichlet --scale --scale-centre 2$", src, re.M)
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert gold.index("t = d_scale[") < gold.index("(real_t)(2) * c[0]") < gold.index("t = t - d_out[") < gold.index("t = t + d_src[") < gold.index("(f != f) ? t : f") and "d_res" not in gold
    # one centre stream serving the centre term and the residual: declared once, loaded once per plane
    assert len(re.findall(r"vec_t cv0_0_0 = vzero;", src)) == 1 and len(re.findall(r"const real_t\* pcen = ", src)) == 1
    kern = src[src.index("void dr_p"):src.index("void res_p")]
    assert len(re.findall(r"cv0_0_0 = ", kern)) == len(re.findall(r"wv0_0_0 = ", kern))
    info = _info(src)
    assert info["scale"] == 1 and info["scale_centre"] == 2 and info["dirichlet"] == 1 and info["source"] == 1 and info["time_order"] == 2 and info["residual"] == "max"
    assert not any(n + "(" in src for n in sc.Emulated.OTHERS)
    h = drs.generate(["--help"])[1]
    assert "--scale " in h and "--scale-centre <c>" in h and "heterogeneous diffusion" in h and "velocity model" in h and "variable diagonal" in h


@pytest.mark.parametrize("extra,reason", [
    (["--step", "2"], "--scale needs --step 1 (a fused S^n scaled once is not n scaled steps)"),
    (["--step", "2", "--temporal", "1"], "--scale needs --step 1"),
    (["--temporal", "force"], "--scale cannot be combined with --temporal"),
    (["--gpus", "2"], "--scale cannot be combined with --gpus N > 1"),
    (["--pair-launch", "1"], "--scale cannot be combined with --pair-launch 1"),
])
def test_cli_scale_rejections(tmp_path, extra, reason):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + SCALE + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", (p.returncode, p.stdout)
    assert reason in p.stderr, p.stderr
    assert not os.path.exists(out)
    p = _cli(["--3d", "--dtype", "fp32"] + extra + ["-o", out, stc], tmp_path)          # legal without the option
    assert p.returncode == 0, p.stdout + p.stderr


def test_cli_scale_centre_needs_scale(tmp_path):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    for c in ("1", "0"):
        p = _cli(["--3d", "--dtype", "fp32", "--scale-centre", c, "-o", out, stc], tmp_path)
        assert p.returncode == 255 and p.stdout == "Invalid configuration!\n" and "--scale-centre needs --scale" in p.stderr, (p.returncode, p.stdout, p.stderr)
    for bad in ("nan", "inf", "-inf", "1x", "x"):               # a finite real, the whole word
        p = _cli(["--3d", "--dtype", "fp32", "--scale", "--scale-centre", bad, "-o", out, stc], tmp_path)
        assert p.returncode == 255 and p.stdout == "Illegal input.\n", (bad, p.returncode, p.stdout)
    assert not os.path.exists(out)


def test_slab_forms_refuse_scale(tmp_path):
    from drstencil_amd import multigpu
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    opts = ["--3d", "--dtype", "fp32"] + SCALE
    with pytest.raises(ValueError, match="--scale"):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match="--scale"):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match="--scale"):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match="--scale"):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    with pytest.raises(drs.KernelBuildError, match="--scale is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))


def test_bare_c4_scale_keeps_the_tuned_row():
    """--scale names the problem: a bare C4 command line still takes the tuner's step-1 row, and the kernel info's register demand grows
    by the scale stream's RY * VX * (PD + 1) words (twice that in fp64); a centre term adds the centre sets, which --residual max has
    already: with both they are counted once."""
    args = ["--3d", "--dtype", "fp32"]
    rc0, msg0, src0 = drs.generate(args + ["--step", "1", C4])
    rc1, msg1, src1 = drs.generate(args + SCALE + [C4])
    rc2, msg2, src2 = drs.generate(args + SCALE + ["--scale-centre", "1", C4])
    assert rc0 == rc1 == rc2 == 0
    row = re.search(r"is used \((.*?)\)", msg0).group(1)
    assert "is used (%s)" % row in msg1 and "is used (%s)" % row in msg2
    i0, i1, i2 = _info(src0), _info(src1), _info(src2)
    assert "wv1_0_0" in src1 and "wv2_0_0" not in src1 and "scale" not in i0 and "cv0_0_0" not in src1 and "cv1_0_0" in src2
    sets = i0["points_per_lane"] * 2
    assert i1["reg_demand"] == i0["reg_demand"] + sets and i2["reg_demand"] == i0["reg_demand"] + 2 * sets
    base = ["--3d", "--dtype", "fp64", "--sn", "8", "--prefetch"]
    j = {k: _info(drs.generate(base + x + [rc.stc("t3_star")])[2])["reg_demand"]
         for k, x in (("plain", []), ("scale", SCALE), ("centre", SCALE + ["--scale-centre", "1"]), ("res", rc.RES), ("res_scale", rc.RES + SCALE),
                      ("res_centre", rc.RES + SCALE + ["--scale-centre", "1"]))}
    w = 2 * _info(drs.generate(base + [rc.stc("t3_star")])[2])["points_per_lane"] * 2
    assert j["scale"] == j["plain"] + w and j["centre"] == j["plain"] + 2 * w
    assert j["res_scale"] == j["res"] + w and j["res_centre"] == j["res_scale"]              # one family of centre sets


def test_no_trace_without_scale():
    """A command line without --scale emits no trace of the option (the corpus of scripts/emit_corpus.py pins the whole text)."""
    seen = 0
    older = GPU_SMALL[::5] + [("c4", 3, C4, ["--3d", "--dtype", "fp32", "--step", "2"]),
                              ("src", 3, rc.stc("t3_wave"), ["--3d", "--source", "--time-order", "2", "--store-mask", "buffer", "--residual", "max", "--dirichlet"])]
    for cid, ndim, stc, opts in older:
        rc_, msg, src = drs.generate(opts + [stc])
        assert src is None or not any(w in src for w in ("pscl", "wv0_", "d_scale", "\"scale", "per-cell factor", "_ops(")), cid
        seen += src is not None
        if src is not None and "--step" not in opts:
            rc_, msg, src = drs.generate(opts + SCALE + [stc])
            assert rc_ == 0 and "pscl" in src and _info(src)["scale"] == 1, cid
    assert seen >= 6


# ---- 10. the C ABI's refusals (nothing is launched: the kernels are cross-compiled and loaded) ----------------------------------------
def test_abi_refusals():
    import ctypes
    cid, ndim, stc, opts = sc.EDGE[1]
    L = drs.lib()
    kscl = drs.Kernel(sc.with_scale(opts, 1) + [stc])
    kplain = drs.Kernel(list(opts) + [stc])
    ksrc = drs.Kernel(list(opts) + sc.SOURCE + [stc])
    kfix = drs.Kernel(list(opts) + sc.DIR + [stc])
    kres = drs.Kernel(list(opts) + rc.RES + [stc])
    assert kscl.scale and kscl.scale_centre == 1.0 and kscl.info["scale"] == 1 and not kplain.scale and kplain.scale_centre == 0.0 and "scale" not in kplain.info
    assert kscl.bytes_per_launch() == kplain.bytes_per_launch() * 3 // 2               # the centre re-read is cached: not counted
    ms = ctypes.c_float()
    # every existing launch or run entry point on a --scale kernel
    assert L.drs_kernel_launch(kscl.h, 1, 2, 0) == -2 and L.drs_kernel_launch_gold(kscl.h, 1, 2, 0) == -2
    assert L.drs_kernel_run(kscl.h, 1, 2, 4, 0, 0) == -2 and L.drs_kernel_run_timed(kscl.h, 1, 2, 4, 0, 0, ms) == -2
    assert L.drs_kernel_launch_src(kscl.h, 1, 2, 3, 0) == -2 and L.drs_kernel_launch_gold_src(kscl.h, 1, 2, 3, 0) == -2
    assert L.drs_kernel_run_src(kscl.h, 1, 2, 3, 4, 0, 0) == -2 and L.drs_kernel_run_timed_src(kscl.h, 1, 2, 3, 4, 0, 0, ms) == -2
    assert L.drs_kernel_launch_res(kscl.h, 1, 2, None, 4, 0) == -2 and L.drs_kernel_run_res(kscl.h, 1, 2, None, 4, 4, 0) == -2
    assert L.drs_kernel_solve(kscl.h, 1, 2, None, 4, 1e-3, 8, 1, 0, None, None) == -2
    assert L.drs_kernel_launch_fix(kscl.h, 1, 2, None, None, 5, 0) == -2 and L.drs_kernel_launch_gold_fix(kscl.h, 1, 2, None, 5, 0) == -2
    assert L.drs_kernel_run_fix(kscl.h, 1, 2, None, None, 5, 4, 0, 0) == -2 and L.drs_kernel_run_timed_fix(kscl.h, 1, 2, None, None, 5, 4, 0, 0, ms) == -2
    assert L.drs_kernel_solve_fix(kscl.h, 1, 2, None, 4, 5, 1e-3, 8, 1, 0, None, None) == -2

    def ops(src=None, res=None, fix=None, scale=None, size=None):
        return ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands) if size is None else size, src, res, fix, scale))

    def every(k, o, want=-2):
        assert L.drs_kernel_launch_ops(k.h, 1, 2, o, 0) == want and L.drs_kernel_run_ops(k.h, 1, 2, o, 4, 0, 0) == want
        assert L.drs_kernel_run_timed_ops(k.h, 1, 2, o, 4, 0, 0, ms) == want
        assert L.drs_kernel_solve_ops(k.h, 1, 2, o, 1e-3, 8, 1, 0, None, None) == want
    # a missing operand, a superfluous one, a wrong size, no block at all -- on every kind of kernel
    need = {kplain: {}, ksrc: {"src": 3}, kfix: {"fix": 5}, kres: {"res": 4}, kscl: {"scale": 6}}
    for k, good in need.items():
        for name in good:
            every(k, ops(**{n: v for n, v in good.items() if n != name}))
        for name, v in (("src", 3), ("res", 4), ("fix", 5), ("scale", 6)):
            if name not in good:
                every(k, ops(**dict(good, **{name: v})))
                if name != "res":
                    assert L.drs_kernel_launch_gold_ops(k.h, 1, 2, ops(**dict(good, **{name: v})), 0) == -2
        every(k, ops(size=8, **good))
        every(k, ops(size=ctypes.sizeof(drs.Operands) + 8, **good))
        every(k, None)
        assert L.drs_kernel_launch_gold_ops(k.h, 1, 2, ops(size=0, **good), 0) == -2
        if k is not kres:
            assert L.drs_kernel_solve_ops(k.h, 1, 2, ops(**good), 1e-3, 8, 1, 0, None, None) == -2      # a good block, but no --residual max
    assert L.drs_kernel_solve_ops(kres.h, 1, 2, ops(res=4), 1e-3, 8, 0, 0, None, None) == -2           # check_every < 1
    # Python: the argument checks of d_scale are those of d_fix
    for call in (kscl.launch, kscl.launch_gold, kscl.run, kscl.run_timed):
        with pytest.raises(ValueError, match="needs d_scale"):
            call(1, 2)
    for call in (kplain.launch, kplain.launch_gold, kplain.run, kplain.run_timed):
        with pytest.raises(ValueError, match="without --scale"):
            call(1, 2, d_scale=3)
    with pytest.raises(ValueError):
        kscl.solve(1, 2, None, 1e-3, 8, d_scale=5)
    with pytest.raises(ValueError, match="without --scale"):
        kplain.solve(1, 2, None, 1e-3, 8, d_scale=5)
    with pytest.raises(ValueError, match="without --source"):
        kscl.launch(1, 2, d_scale=5, d_src=3)
    with pytest.raises(ValueError, match="without --dirichlet"):
        kscl.launch(1, 2, d_scale=5, d_fix=3)


# ---- 1. bit-exactness -----------------------------------------------------------------------------------------------------------------
_EXACT = sc.CASES + sc.MODES + sc.FORMS


@pytest.mark.parametrize("cid,ndim,src,opts,c", _EXACT, ids=[c[0] for c in _EXACT])
def test_emulated_scale_cases(tmp_path, monkeypatch, cid, ndim, src, opts, c):
    stc = _case_stc(tmp_path, cid, ndim, src)
    full = sc.with_scale(opts, c)
    lib = sc.build_emulated(tmp_path, stc, full)
    assert lib.info["scale"] == 1 and lib.info["scale_centre"] == c and lib.info["stages"] == 1
    if cid.startswith(sc.BIG[0] + "_c"):
        assert lib.info["stream_blocks"] == 9 and lib.info["tiles_x"] * lib.info["tiles_y"] == 18 and lib.info["grid"] == 168
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W = sc.inputs(spec, full)
    wi = rc.interior(W, spec.halo)
    assert (wi < 0).any() or wi.size == 1
    assert (np.abs(wi) > 1).any() or wi.size == 1                          # on the inputs alone: both signs, magnitudes above 1
    _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, full, A0, B0, F0, X, W, cid)


# ---- 2. unit scale changes nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", sc.UNCHANGED, ids=[c[0] for c in sc.UNCHANGED])
def test_emulated_unit_scale_equals_the_plain_command(tmp_path, cid, ndim, src, opts):
    stc = _case_stc(tmp_path, cid, ndim, src)
    with_opt = sc.build_emulated(tmp_path, stc, sc.with_scale(opts))
    plain = sc.build_emulated(tmp_path, stc, list(opts))
    assert not plain.scale and "scale" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W = sc.inputs(spec, opts)
    W[...] = 1.0
    A1, B1, A2, B2 = A0.copy(), B0.copy(), A0.copy(), B0.copy()
    for t in range(2):
        a, b = ((A1, B1), (B1, A1))[t]
        assert with_opt.launch(a, b, F0, None, None, W) == 0
        a, b = ((A2, B2), (B2, A2))[t]
        assert plain.launch(a, b, F0) == 0
        assert bit_equal(A1, A2) and bit_equal(B1, B2), (cid, t)


# ---- 3. frozen field ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", sc.FROZEN, ids=[c[0] for c in sc.FROZEN])
def test_emulated_frozen_field(tmp_path, cid, ndim, src, opts):
    """w = 0 and centre 1 on inputs without zeros or non-finite values: out equals in on the interior, in bits, and out's ring is untouched."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    full = sc.with_scale(opts, 1)
    lib = sc.build_emulated(tmp_path, stc, full)
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    A0, B0, F0, X, W = sc.inputs(spec, full)
    assert np.isfinite(A0).all() and (A0 != 0).all()
    W[...] = 0.0
    Ar, Br = A0.copy(), B0.copy()
    sc.host_launch(spec, ndim, full, Ar, Br, None, None, W)
    want = B0.copy()
    rc.interior(want, H)[...] = rc.interior(A0, H)
    assert bit_equal(Br, want) and bit_equal(Ar, A0)                       # on the reference alone
    for gold in (False, True):
        A, B = A0.copy(), B0.copy()
        assert (lib.gold(A, B, None, None, W) if gold else lib.launch(A, B, None, None, None, W)) == 0
        assert bit_equal(B, want) and bit_equal(A, A0), (cid, gold, count_different(B, want))


# ---- 4. planted factors -------------------------------------------------------------------------------------------------------------
def _bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def _planted(spec, info, dt):
    cells = rc.planted_cells(info)
    planted = np.zeros(spec.shape, bool)
    vals = np.ones(spec.shape, dt)
    for n, c in enumerate(cells):
        planted[c] = True
        vals[c] = 2 + n / 64
    return cells, planted, vals


@pytest.mark.parametrize("cid,ndim,src,opts", sc.PLANT, ids=[c[0] for c in sc.PLANT])
def test_emulated_planted_factors(tmp_path, cid, ndim, src, opts):
    """w = 1 except at the interior corners and both sides of every x, y and z seam, each with a factor 2 + n/64 of its own; then the
    complement.  Every cell equals the reference in bits, and the cells that differ from the unit-scale run are exactly the planted ones."""
    stc = shutil.copy(src, str(tmp_path))
    full = sc.with_scale(opts)
    lib = sc.build_emulated(tmp_path, stc, full)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, _ = sc.inputs(spec, full)
    cells, planted, vals = _planted(spec, lib.info, A0.dtype)
    assert len(cells) >= (14 if cid.startswith(sc.BIG[0]) else 10), (cid, len(cells))
    inner = ~ring_mask(spec.shape, spec.halo)
    unit = B0.copy()
    sc.host_launch(spec, ndim, full, A0.copy(), unit, None, None, np.ones(spec.shape, A0.dtype))
    every = (2 + (np.arange(planted.size).reshape(planted.shape) % 64) / 64).astype(A0.dtype)
    for mask, W in ((planted, vals), (~planted & inner, np.where(~planted & inner, every, 1).astype(A0.dtype))):
        Br = B0.copy()
        sc.host_launch(spec, ndim, full, A0.copy(), Br, None, None, W)
        assert np.array_equal(_bits(Br) != _bits(unit), mask), (cid, int(mask.sum()))                    # on the reference alone
        A, B = _launches(lib, spec, ndim, full, A0, B0, None, None, W, (cid, int(mask.sum())), launches=1)
        assert np.array_equal(_bits(B) != _bits(unit), mask), (cid, int(mask.sum()))
        _launches(lib, spec, ndim, full, A0, B0, None, None, W, (cid, int(mask.sum()), "gold"), launches=1, gold=True)


# ---- 5. no contraction ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", sc.CONTRACTION, ids=[c[0] for c in sc.CONTRACTION])
def test_emulated_no_contraction(tmp_path, cid, ndim, src, opts):
    """Centre 0.3: a kernel that contracted w * v + t or C * in + (w * v) into an FMA would differ from the contract in at least one cell
    (asserted on the reference alone: fp32 through exact float64 products, fp64 in rationals on a few hundred cells); the kernel equals
    the contract in bits.  (The two centre statements emitted as one FMA, tried once by hand in emit_centre_term and in the gold kernel,
    fail all four cases here, the ten centre-0.3 entries of test_emulated_scale_cases and the centre-0.3 half of the memory contract; the
    centre-1 and centre-2 entries pass, since C * in is exact there.)"""
    stc = _case_stc(tmp_path, cid, ndim, src)
    full = sc.with_scale(opts, 0.3)
    lib = sc.build_emulated(tmp_path, stc, full)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W = sc.inputs(spec, full)
    shape_i = rc.interior(A0, spec.halo).shape
    cells = None
    if A0.dtype == np.float64:
        cells = np.zeros(shape_i, bool)
        cells.reshape(-1)[np.random.default_rng(3).choice(cells.size, 300, replace=False)] = True
    Br = B0.copy()
    sc.host_launch(spec, ndim, full, A0.copy(), Br, None, None, W)
    for variant in ("fma_w", "fma_c"):
        Bv = Br.copy()                                                    # outside `cells` the contract's values stand
        sc.host_launch(spec, ndim, full, A0.copy(), Bv, None, None, W, variant=variant, cells=cells)
        assert count_different(Bv, Br) >= 1, (cid, variant, "the contracted variant equals the contract on this seed")
    A, B = _launches(lib, spec, ndim, full, A0, B0, None, None, W, cid, launches=1)
    assert bit_equal(B, Br)
    _launches(lib, spec, ndim, full, A0, B0, None, None, W, (cid, "gold"), launches=1, gold=True)


# ---- 6. special values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("held", [False, True], ids=["free", "dirichlet"])
@pytest.mark.parametrize("cid,ndim,src,opts", sc.SPECIAL, ids=[c[0] for c in sc.SPECIAL])
def test_emulated_special_values(tmp_path, cid, ndim, src, opts, held):
    """w holds +0.0, -0.0, +-inf, NaN and the smallest subnormals at corners and seams; `in` is planted so that S(in) is inf where w = 0
    (-> NaN), -0.0 where w = -0.0 and finite where w = inf.  NaN where the reference is NaN, bits elsewhere; with --dirichlet a held cell
    whose scaled value is NaN still stores fix[p]."""
    stc = shutil.copy(src, str(tmp_path))
    full = sc.with_scale(list(opts) + (sc.DIR if held else []), 1)
    lib = sc.build_emulated(tmp_path, stc, full)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W, cells = sc.special_problem(spec, full, lib.info)
    _special_sites(spec, ndim, full, A0, B0, X, W, cells, held)
    for gold in (False, True):
        _launches(lib, spec, ndim, full, A0, B0, None, X, W, (cid, held, gold), launches=2, gold=gold)


def _special_sites(spec, ndim, full, A0, B0, X, W, cells, held):
    """The built sites, asserted on the reference alone."""
    S = B0.copy()
    oracle.sweep(spec, A0.copy(), S, contract=1)
    Br = B0.copy()
    sc.host_launch(spec, ndim, full, A0.copy(), Br, None, X, W)
    p, q, s = cells["zero_times_inf"], cells["inf_times_fin"], cells["m0_times_m0"]
    m0 = np.asarray(-0.0, A0.dtype).tobytes()
    assert np.isinf(S[p]) and W[p] == 0 and (Br[p] == 0.5 if held else np.isnan(Br[p]))
    assert np.isfinite(S[q]) and S[q] != 0 and np.isinf(W[q]) and np.isinf(Br[q])
    assert S[s].tobytes() == m0 and W[s].tobytes() == m0
    wi = rc.interior(W, spec.halo)
    for v in sc.w_specials(A0.dtype):
        assert (np.isnan(wi).any() if np.isnan(v) else (wi.view(np.uint32) == np.asarray(v).view(np.uint32)).any()), v
    return Br


# ---- 7. memory contract and read log --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", sc.CONTRACT, ids=[c[0] for c in sc.CONTRACT])
def test_scale_memory_contract(tmp_path, cid, ndim, src, opts):
    """in, out, src, w (and d_res) each flush against PROT_NONE pages (end-flush and start-flush), in a child process: no SIGSEGV, exact
    arrays, out's ring unchanged, w unwritten and its garbage ring without effect."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    for o in (sc.with_scale(opts, 2), sc.with_scale(list(opts) + sc.SOURCE + rc.RES, 0.3)):
        lib = sc.build_emulated(tmp_path, stc, o)
        job = {"so": lib.so, "stc": stc, "ndim": ndim, "opts": o, "placements": ["end", "start"]}
        jpath = str(tmp_path / "job.json")
        with open(jpath, "w") as f:
            json.dump(job, f)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scale_child.py"), jpath], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (o, p.returncode, p.stdout[-1500:], p.stderr[-1500:])


@pytest.mark.parametrize("cid,ndim,src,opts", sc.READLOG, ids=[c[0] for c in sc.READLOG])
def test_scale_read_log(tmp_path, cid, ndim, src, opts):
    """With tests/source_readlog.h in front and the watch laid over w, one launch reads every interior byte of w and no ring byte."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    full = sc.with_scale(opts, 1)
    lib = sc.build_emulated(tmp_path, stc, full, read_log=True)
    spec = oracle.Spec(stc, ndim, 1)
    A, B, F, X, W = sc.inputs(spec, full)
    seen = np.zeros(W.nbytes, np.uint8)
    lib.lib.drs_readlog_watch(W.ctypes.data, W.nbytes, seen.ctypes.data)
    assert lib.launch(A, B, F, None, X, W) == 0
    lib.lib.drs_readlog_watch(None, 0, None)
    seen = seen.reshape(spec.shape + (W.itemsize,))
    ring = ring_mask(spec.shape, spec.halo)
    assert seen[~ring].all(), (cid, "interior bytes of w not read", int((seen[~ring] == 0).sum()))
    assert not seen[ring].any(), (cid, "ring bytes of w read", int(seen[ring].sum()))


# ---- 8. the samples of the tuner's space ----------------------------------------------------------------------------------------------
SMALL_GRID = {3: (13, 21, 300), 2: (1, 37, 300)}       # tiny ragged grids: more than one stream block, a partial x-edge tile
_SAMPLE = [(w, n, j) for w in sc.SAMPLES for n, j in enumerate(sc.sample_jobs(w))]


@pytest.mark.parametrize("which,n,job", _SAMPLE, ids=["%s-%02d" % (w, n) for w, n, _ in _SAMPLE])
def test_emulated_scale_sampled_fuzz(tmp_path, monkeypatch, which, n, job):
    """The samples on tiny grids.  What the generator refuses there it refuses without --scale too, for its own reason."""
    ndim, path, dtype, args, step = job
    opts = args[:-1]
    assert "--scale" in opts and step == 1
    stc = _small_stc(tmp_path, path, ndim, SMALL_GRID[ndim])
    p = _cli(opts + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
    if p.returncode != 0:
        q = _cli(sc.plain_opts(opts) + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
        assert p.returncode == 255 and q.returncode == 255 and "--scale" not in p.stderr, (p.stderr, q.stderr)
        return
    lib = sc.build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, step)
    A0, B0, F0, X, W = sc.inputs(spec, opts)
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, (which, n, "forward"))
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _launches(_second_lib(lib, tmp_path, "rev"), spec, ndim, opts, A0, B0, F0, X, W, (which, n, "reverse"))


def test_scale_sample_size():
    for w in sc.SAMPLES:
        jobs = sc.sample_jobs(w)
        assert len(jobs) == sc.SAMPLE_SIZE == 20 and jobs == sc.sample_jobs(w) and all("--scale" in j[3] for j in jobs)
        assert all(("--source" in j[3] and "--time-order" in j[3] and j[3][-3:-1] == ["--scale-centre", "2"]) == (w != "scale") for j in jobs)
        assert len(sc.REFUSED[w]) <= sc.SAMPLE_SIZE - sc.MIN_CHECKED == 5


# ---- 9. run to tolerance --------------------------------------------------------------------------------------------------------------
def _emulated_solve(lib, A, B, F, X, W, tol, max_launches, check_every):
    """drs_kernel_solve_ops' loop on an emulated plugin: the library's own loop needs a device; its decisions are these."""
    n, r = 0, None
    limit = max_launches - max_launches % 2
    res = _nan_res(lib, A.dtype)
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            assert lib.launch(A, B, F, res, X, W) == 0 and lib.launch(B, A, F, res, X, W) == 0
            n += 2
        r = res[0]
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r


_SOLVE = [(c[0] + ("_held" if h else ""), c[1], c[2], c[3], c[4], h) for c in sc.SOLVE for h in (False, True)]


@pytest.mark.parametrize("cid,ndim,src,opts,tol,held", _SOLVE, ids=[c[0] for c in _SOLVE])
def test_emulated_run_to_tolerance(tmp_path, cid, ndim, src, opts, tol, held):
    """Screened Poisson -Lap u + sigma u = 1 on 10^3 with a ring of 0, as the Jacobi sweep u' = w * S(u) + src with w = 6 / (6 + sigma),
    src = 1 / (6 + sigma): status, launch count, r, both arrays and w equal a numpy loop of the host reference that looks at r at the same
    launches (check_every = 4 pairs); once more with an inner block held through fix.  The screening makes the sweep a stronger
    contraction: fewer launches than the same problem with sigma = 0 (asserted on the reference alone)."""
    stc = rc.solve_stc(tmp_path, "emu", ndim, src)
    o = sc.solve_opts(opts, held)
    lib = sc.build_emulated(tmp_path, stc, o)
    spec = oracle.Spec(stc, ndim, 1)
    dt = sc.dtype_of(opts)
    A, B, F, X, W = sc.solve_problem(spec, dt, held=held)
    Ar, Br = A.copy(), B.copy()
    want = sc.oracle_solve(spec, Ar, Br, F, X, W, tol, sc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and want[1] < sc.MAX_LAUNCHES and want[1] % 8 == 0, want
    A1, B1, F1, X1, W1 = sc.solve_problem(spec, dt, sigma=False, held=held)
    assert (W1 == 1).all()
    unscreened = sc.oracle_solve(spec, A1, B1, F1, X1, W1, tol, sc.MAX_LAUNCHES, 4)
    assert unscreened[0] == 0 and want[1] < unscreened[1], (want, unscreened)
    W0 = W.copy()
    got = _emulated_solve(lib, A, B, F, X, W, tol, sc.MAX_LAUNCHES, 4)
    print(cid, "launches", got[1], "residual", got[2], "sigma = 0:", unscreened[1])
    assert got[0] == 0 and got[1] == want[1] and rc.same_bits(got[2], want[2]), (got, want)
    assert bit_equal(A, Ar) and bit_equal(B, Br) and bit_equal(W, W0)
    if held:
        h = ~np.isnan(X)
        assert bit_equal(A[h], X[h]) and bit_equal(B[h], X[h])
    assert A.min() >= 0.0 and rc.interior(A, spec.halo).max() > 0.01
    # max_launches = 17: status 1 with 16 launches
    A, B, F, X, W = sc.solve_problem(spec, dt, held=held)
    assert _emulated_solve(lib, A, B, F, X, W, tol, 17, 4)[:2] == (1, 16)
