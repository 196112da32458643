"""--varcoef (one coefficient array per tap: out = sum_t a_t[p] * in[p + d_t]) without a GPU: the generator's option surface and fit rule,
the C ABI's refusals, and the emitted kernels under the CPU emulation (tests/emu) in both fiber orders -- whole arrays bit for bit against
the host reference of tests/varcoef_cases.py (the gold-order chain with libm's correctly rounded fma), constant arrays against the same
command without the option, exact small integers against integer numpy, tap identity, IEEE special values in the coefficients, the
memory contract flush against inaccessible pages with a read log over coef, the sample of the tuner's space and the run to tolerance on
-div(kappa grad u) = f.

The case list is tests/varcoef_cases.py's, the one tests/test_varcoef_gpu.py runs on the GPU.  The knob cases on t3_star run that stencil
on smaller grids here (more than one tile and stream block, partial tiles), so that each takes seconds under the emulation; the
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
import scale_cases as sc
import varcoef_cases as vc
from emu_util import DRSTENCIL
from footprint import bit_equal, ring_mask
from gpu_cases import SMALL as GPU_SMALL
from helpers import write_stc
from special_values import count_different, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "benchmarks", "configs")
VC = vc.VC
# grids of the emulated knob cases: (L, M, N)
DIMS = {"prefetch_depth2": (19, 37, 264), "defer_stores": (13, 19, 264), "rows_unpacked": (21, 19, 264), "cyclic_merge_x2_fp64": (13, 19, 140),
        "loader_waves_fp64": (13, 19, 140), "store_mask_buffer": (13, 37, 264), "odd_elem_fp64": (13, 21, 135), "tile_2d_fp32": (1, 41, 268),
        "tile_2d_box9_fp64": (1, 41, 140), "stream_2d_fp32": (1, 61, 268), "stream_2d_dma_fp64": (1, 45, 140),
        "ahead_3d": (21, 23, 140), "ahead_2d": (1, 61, 268), "shape_11": (19, 21, 139), "shape_05": (17, 21, 76), "box25_2d": (1, 45, 140),
        "identity_lap3": (11, 13, 76), "identity_lap2": (1, 25, 140)}


def _cli(args, cwd):
    return subprocess.run([DRSTENCIL] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


def _small_stc(tmp_path, src, ndim, dims, name=None):
    pts = [tuple(off[3 - ndim:]) + (c,) for off, c in oracle.Spec(src, ndim, 1).points]
    path = os.path.join(str(tmp_path), (name or os.path.basename(src)[:-4]) + ".stc")
    write_stc(path, ndim, dims, 4, pts)
    return path


def _case_stc(tmp_path, cid, ndim, src):
    g = next((k for k in DIMS if cid.startswith(k)), None)
    return _small_stc(tmp_path, src, ndim, DIMS[g]) if g else shutil.copy(src, str(tmp_path))


def _info(src):
    return json.loads(re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', src).group(1).replace('\\"', '"'))


def _second_lib(lib, tmp_path, tag):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    cp = os.path.join(str(tmp_path), tag + "_" + os.path.basename(lib.so))
    shutil.copy(lib.so, cp)
    return vc.load_emulated(cp)


def _nan_res(lib, dt):
    return np.full(lib.residual_elems, np.nan, dt) if lib.residual_elems else None


def _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, K, what, launches=3, gold=False):
    """`launches` launches from (A0, B0): after each, both WHOLE arrays equal the host reference's in bits; with --residual max r equals
    numpy's in bits and every element of the NaN-filled residual array has been overwritten.  Afterwards coef, w, src and fix are
    bit-unchanged."""
    A, B = A0.copy(), B0.copy()
    Ar, Br = A0.copy(), B0.copy()
    keep = [None if a is None else a.copy() for a in (F0, X, W, K)]
    for t in range(launches):
        s, d = (A, B) if t % 2 == 0 else (B, A)
        sr, dr = (Ar, Br) if t % 2 == 0 else (Br, Ar)
        res = None if gold else _nan_res(lib, A.dtype)
        assert (lib.gold(s, d, F0, X, W, K) if gold else lib.launch(s, d, F0, res, X, W, K)) == 0
        want = vc.host_launch(spec, ndim, opts, sr, dr, F0, X, W, K)
        assert same_bits(A, Ar) and same_bits(B, Br), (what, t, count_different(A, Ar), count_different(B, Br))
        if res is not None:
            assert rc.same_bits(res[0], want), (what, t, res[0], want)
            assert not np.isnan(res).any() or np.isnan(want), (what, t, "partials not written")
    for a, k in zip((F0, X, W, K), keep):
        assert a is None or bit_equal(a, k), (what, "src, fix, w or coef was written")
    return A, B


def _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, opts, A0, B0, F0, X, W, K, what, launches=3, tag="rev"):
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, K, (what, "forward"), launches)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, K, (what, "gold"), launches, gold=True)
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _launches(_second_lib(lib, tmp_path, tag), spec, ndim, opts, A0, B0, F0, X, W, K, (what, "reverse"), launches)


# ---- interface: generator / CLI -------------------------------------------------------------------------------------------------------
def test_cli_varcoef(tmp_path):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (10, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + VC + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "coef" not in p.stdout                                             # stdout stays the reference's protocol
    notes = [ln for ln in p.stderr.splitlines() if "per-tap coefficients" in ln]
    assert len(notes) == 1 and notes[0].startswith("drstencil: note: per-tap coefficients: a launch takes one more array coef of 7 grids")
    src = open(out).read()
    info = _info(src)
    spec = oracle.Spec(stc, 3, 1)
    assert info["varcoef"] == 1 and info["coef_taps"] == [list(o) for o, _ in spec.points] and len(info["coef_taps"]) == info["taps"] == 7
    assert "scale" not in info and "source" not in info
    # (no geometry option: the fit rule has spelled a smaller geometry out, in front of the option's canonical place)
    assert re.search(r"^// options: --3d --dtype fp32 -o \S+ --bx 64 --by 4 --block-merge-x 4 --block-merge-y \d --sn 8 --tuned-defaults 0 --varcoef$", src, re.M)
    assert "stepped down to --bx 64 --by 4 --block-merge-x 4 --block-merge-y" in p.stderr
    assert "const real_t* __restrict__ d_in, real_t* __restrict__ d_out, const real_t* __restrict__ d_coef)" in src
    assert "drs_plugin_launch_ops(const void* in, void* out, const void* src, void* res, const void* fix, const void* scale, const void* coef, hipStream_t stream)" in src
    assert "drs_plugin_launch_gold_ops(const void* in, void* out, const void* src, const void* fix, const void* scale, const void* coef, hipStream_t stream)" in src
    assert not any(n + "(" in src for n in sc.Emulated.OTHERS)
    # the .stc constants are not used by either kernel
    kern = src[src.index("void dr_p"):src.index("void gold_p")]
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert "(real_t)(0." not in kern and "(real_t)(0." not in gold
    assert "real_t t = a[0L * DRS_COEF_GRID] * c[" in gold and "__builtin_fmaf(a[6L * DRS_COEF_GRID], c[" in gold
    assert "#define DRS_COEF_GRID ((long)L * M * N)" in src and "pcoef += DRS_STRIDE_S;" in src
    assert all("vec_t kv%d_0_0_0 = vzero;" % t in src for t in range(7)) and "kv7_" not in src and "kv0_1_" not in src      # one set per tap
    rc2, msg, src2 = drs.generate(["--3d", "--dtype", "fp32"] + VC + ["-o", out, stc])
    assert rc2 == 0 and src2 == src and "drstencil: note: per-tap coefficients:" in msg
    # one place in the banner, behind every other option, wherever and however often it stands
    rc3, msg3, src3 = drs.generate(["--varcoef", "--3d", "--varcoef", "--dtype", "fp32", "-o", out, stc])
    assert rc3 == 0 and src3 == src
    # with every other array: in, out, src, res, fix, w, coef; gold without res
    p = _cli(["--3d", "--dtype", "fp32", "--varcoef", "--source", "--time-order", "2", "--residual", "max", "--dirichlet", "--scale", "--scale-centre", "2", "-o", out, stc], tmp_path)
    src = open(out).read()
    assert p.returncode == 0 and ("real_t* __restrict__ d_out, const real_t* __restrict__ d_src, real_t* __restrict__ d_res, const real_t* __restrict__ d_fix, "
                                  "const real_t* __restrict__ d_scale, const real_t* __restrict__ d_coef)") in src
    assert "(const real_t*)in, (real_t*)out, (const real_t*)src, (real_t*)res, (const real_t*)fix, (const real_t*)scale, (const real_t*)coef);" in src
    assert re.search(r"--dirichlet --scale --scale-centre 2 --varcoef$", src, re.M)
    gold = src[src.index("void gold_p"):src.index("extern \"C\" int drs_plugin")]
    assert gold.index("a[6L * DRS_COEF_GRID]") < gold.index("t = d_scale[") < gold.index("t = t - d_out[") < gold.index("t = t + d_src[") < gold.index("(f != f) ? t : f")
    info = _info(src)
    assert info["varcoef"] == 1 and info["scale"] == 1 and info["dirichlet"] == 1 and info["source"] == 1 and info["time_order"] == 2 and info["residual"] == "max"
    # 2D: (j, i) offsets with k = 0
    s2 = _small_stc(tmp_path, rc.stc("t2_star"), 2, (1, 20, 24), name="q")
    for extra in ([], ["--streaming"]):
        rc4, _, src4 = drs.generate(["--dtype", "fp64"] + extra + VC + [s2])
        assert rc4 == 0 and _info(src4)["coef_taps"] == [list(o) for o, _ in oracle.Spec(s2, 2, 1).points] and "#define DRS_COEF_GRID ((long)M * N)" in src4
    h = drs.generate(["--help"])[1]
    assert "--varcoef " in h and "heterogeneous diffusion  u' = u + dt*div(k grad u)" in h and "anisotropic operator" in h and "Jacobi, stencil-form A" in h


@pytest.mark.parametrize("extra,reason", [
    (["--step", "2"], "--varcoef needs --step 1 (a fused S^n with coefficients taken at one cell is not n variable-coefficient steps)"),
    (["--step", "2", "--temporal", "1"], "--varcoef needs --step 1"),
    (["--temporal", "force"], "--varcoef cannot be combined with --temporal"),
    (["--gpus", "2"], "--varcoef cannot be combined with --gpus N > 1"),
    (["--pair-launch", "1"], "--varcoef cannot be combined with --pair-launch 1"),
    (["--coef", "sgpr"], "--varcoef cannot be combined with --coef"),
    (["--order", "rows", "--pack", "1"], "--varcoef cannot be combined with --pack 1"),
])
def test_cli_varcoef_rejections(tmp_path, extra, reason):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + VC + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", (p.returncode, p.stdout)
    assert reason in p.stderr, p.stderr
    assert not os.path.exists(out)
    p = _cli(["--3d", "--dtype", "fp32"] + extra + ["-o", out, stc], tmp_path)          # legal without the option
    assert p.returncode == 0, p.stdout + p.stderr


@pytest.mark.parametrize("ndim,stc,dtype", [(2, os.path.join(ROOT, "benchmarks", "2d25pt_box", "2d25pt_box.stc"), "fp32"), (3, rc.stc("shape_03_3d_o1"), "fp32"),
                                            (3, rc.stc("drift_c34_3d_o1"), "fp64"), (2, rc.stc("t2_box25"), "fp64"), (3, os.path.join(CFG, "c4_3d7pt_star_1024.stc"), "fp32"),
                                            (2, os.path.join(CFG, "c5_2d25pt_box_16384.stc"), "fp64")])
def test_stepped_down_source_is_reproduced_by_its_banner(ndim, stc, dtype):
    """A bare --varcoef command that the fit rule steps down: the banner spells the geometry out once, and the banner's command emits the
    same source, byte for byte -- the planner's default emission order (rows for 3D stencils beyond 25 taps and 2D tiles beyond 9) included."""
    rc_, msg, src = drs.generate((["--3d"] if ndim == 3 else []) + ["--dtype", dtype] + VC + [stc])
    assert rc_ == 0 and "stepped down to" in msg, msg
    words = re.search(r"^// options: (.*)$", src, re.M).group(1).split()
    assert words.count("--bx") == words.count("--by") == 1 and words[-1] == "--varcoef"
    rc2, msg2, src2 = drs.generate(words + [stc])
    assert rc2 == 0 and "stepped down" not in msg2 and src2 == src
    many = len(oracle.Spec(stc, ndim, 1).points) > (25 if ndim == 3 else 9)
    assert _info(src)["order"] == ("rows" if many else "taps")


def test_rows_order_is_unpacked_by_default(tmp_path):
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    rc_, _, src = drs.generate(["--3d", "--dtype", "fp32", "--order", "rows"] + VC + [stc])
    assert rc_ == 0 and _info(src)["packed"] == 0 and _info(src)["order"] == "rows" and "vec2_t" not in src
    rc_, _, src = drs.generate(["--3d", "--dtype", "fp32", "--order", "rows", stc])
    assert rc_ == 0 and _info(src)["packed"] == 1


def test_slab_forms_refuse_varcoef(tmp_path):
    from drstencil_amd import multigpu
    stc = _small_stc(tmp_path, rc.stc("t3_wave"), 3, (16, 12, 16), name="p")
    opts = ["--3d", "--dtype", "fp32"] + VC
    with pytest.raises(ValueError, match="--varcoef"):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match="--varcoef"):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match="--varcoef"):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match="--varcoef"):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    with pytest.raises(drs.KernelBuildError, match="--varcoef is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))


# ---- the fit rule (the cross-compiler only) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", vc.BENCH_CONFIGS)
def test_bare_varcoef_fits(cfg):
    """The bare --varcoef command on every benchmark configuration, fp32 and the .stc's own fp64 for the 25-tap C5: it builds for gfx950
    with no scratch and no spilled scalar registers; where the planned geometry does not hold the coefficient values, one note on stderr
    names the geometry chosen, and the kernel info reports it."""
    stc = os.path.join(CFG, cfg + ".stc")
    ndim = 3 if "_3d" in cfg else 2
    args = (["--3d"] if ndim == 3 else []) + ["--dtype", "fp64" if cfg.startswith("c5") else "fp32"] + VC + [stc]
    rc_, msg, src = drs.generate(args)
    assert rc_ == 0, msg
    info = _info(src)
    notes = [ln for ln in msg.splitlines() if "stepped down to" in ln]
    plain = _info(drs.generate([a for a in args if a != "--varcoef"])[2])
    words = (1 if info["dtype"] == "fp32" else 2) * info["taps"]
    assert info["reg_demand"] - words * info["points_per_lane"] > 0
    if notes:
        assert len(notes) == 1
        geo = re.search(r"stepped down to (--bx (\d+) --by (\d+) --\w+-merge-x (\d+).*)$", notes[0])
        assert geo, notes[0]
        assert info["threads"] == int(geo.group(2)) * (int(geo.group(3)) if info["streams"] == 0 or ndim == 3 else 1)
        assert info["points_per_lane"] < plain["points_per_lane"] or info["threads"] < plain["threads"]
        assert re.search(r"^// options: .*%s.* --varcoef$" % re.escape(geo.group(1)), src, re.M)
    else:
        assert info["points_per_lane"] == plain["points_per_lane"] and info["threads"] == plain["threads"]
    k = drs.Kernel(args)                 # cross-compiles; refuses scratch and spilled scalar registers
    r = k.resources
    print(cfg, "vgprs", r["vgprs"], "agprs", r["agprs"], "sgprs", r["sgprs"], "scratch", r["scratch_bytes_per_lane"], "|", notes[0] if notes else "as planned")
    assert r["scratch_bytes_per_lane"] == 0 and r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0
    assert k.varcoef and len(k.coef_taps) == info["taps"]
    # a geometry given explicitly is taken as given: no step-down
    explicit = [a for a in args[:-1]] + ["--bx", "64", "--by", "4", stc]
    rc_, msg, _ = drs.generate(explicit)
    assert rc_ == 0 and "stepped down" not in msg


def test_varcoef_register_demand(tmp_path):
    """reg_demand grows by T * RY * VX words (twice that in fp64), one set whatever the prefetch depth."""
    for dt, words in (("fp32", 1), ("fp64", 2)):
        for pre in ([], ["--prefetch", "--prefetch-depth", "2"]):
            base = ["--3d", "--dtype", dt, "--sn", "8", "--by", "4", "--block-merge-y", "2"] + pre
            i0 = _info(drs.generate(base + [rc.stc("t3_star")])[2])
            i1 = _info(drs.generate(base + VC + [rc.stc("t3_star")])[2])
            assert i1["reg_demand"] == i0["reg_demand"] + words * 7 * i0["points_per_lane"], (dt, pre)


def test_no_trace_without_varcoef():
    """A command line without --varcoef emits no trace of the option (the corpus of scripts/emit_corpus.py pins the whole text)."""
    seen = 0
    older = GPU_SMALL[::5] + [("c4", 3, os.path.join(CFG, "c4_3d7pt_star_1024.stc"), ["--3d", "--dtype", "fp32", "--step", "2"]),
                              ("all", 3, rc.stc("t3_wave"), ["--3d", "--source", "--time-order", "2", "--store-mask", "buffer", "--residual", "max", "--dirichlet", "--scale", "--scale-centre", "2"])]
    for cid, ndim, stc, opts in older:
        rc_, msg, src = drs.generate(opts + [stc])
        assert src is None or not any(w in src for w in ("pcoef", "kv0_", "d_coef", "varcoef", "DRS_COEF_GRID", "per-tap", "const void* coef")), cid
        seen += src is not None
        if src is not None and "--step" not in opts:
            rc_, msg, src = drs.generate(opts + VC + [stc])
            assert rc_ == 0 and "pcoef" in src and _info(src)["varcoef"] == 1, cid
    assert seen >= 6


# ---- the C ABI's refusals (nothing is launched: the kernels are cross-compiled and loaded) ---------------------------------------------
def test_abi_refusals():
    import ctypes
    cid, ndim, stc, opts = vc.EDGE[1]
    L = drs.lib()
    kvc = drs.Kernel(vc.with_vc(opts) + [stc])
    kplain = drs.Kernel(list(opts) + [stc])
    ksrc = drs.Kernel(list(opts) + vc.SOURCE + [stc])
    kfix = drs.Kernel(list(opts) + vc.DIR + [stc])
    kres = drs.Kernel(list(opts) + rc.RES + [stc])
    kscl = drs.Kernel(list(opts) + sc.SCALE + [stc])
    spec = oracle.Spec(stc, ndim, 1)
    assert kvc.varcoef and kvc.info["varcoef"] == 1 and not kplain.varcoef and kplain.coef_taps == () and "varcoef" not in kplain.info
    assert kvc.coef_taps == tuple(o for o, _ in spec.points)
    assert json.loads(L.drs_kernel_coef_taps(kvc.h).decode()) == [list(t) for t in kvc.coef_taps] and L.drs_kernel_coef_taps(kplain.h) is None
    assert kvc.bytes_per_launch() == kplain.bytes_per_launch() * (2 + 7) // 2
    assert ctypes.sizeof(drs.Operands) == 6 * ctypes.sizeof(ctypes.c_void_p)
    ms = ctypes.c_float()
    # every plain and suffixed entry point on a --varcoef kernel
    assert L.drs_kernel_launch(kvc.h, 1, 2, 0) == -2 and L.drs_kernel_launch_gold(kvc.h, 1, 2, 0) == -2
    assert L.drs_kernel_run(kvc.h, 1, 2, 4, 0, 0) == -2 and L.drs_kernel_run_timed(kvc.h, 1, 2, 4, 0, 0, ms) == -2
    assert L.drs_kernel_launch_src(kvc.h, 1, 2, 3, 0) == -2 and L.drs_kernel_launch_gold_src(kvc.h, 1, 2, 3, 0) == -2
    assert L.drs_kernel_run_src(kvc.h, 1, 2, 3, 4, 0, 0) == -2 and L.drs_kernel_run_timed_src(kvc.h, 1, 2, 3, 4, 0, 0, ms) == -2
    assert L.drs_kernel_launch_res(kvc.h, 1, 2, None, 4, 0) == -2 and L.drs_kernel_run_res(kvc.h, 1, 2, None, 4, 4, 0) == -2
    assert L.drs_kernel_solve(kvc.h, 1, 2, None, 4, 1e-3, 8, 1, 0, None, None) == -2
    assert L.drs_kernel_launch_fix(kvc.h, 1, 2, None, None, 5, 0) == -2 and L.drs_kernel_launch_gold_fix(kvc.h, 1, 2, None, 5, 0) == -2
    assert L.drs_kernel_run_fix(kvc.h, 1, 2, None, None, 5, 4, 0, 0) == -2 and L.drs_kernel_run_timed_fix(kvc.h, 1, 2, None, None, 5, 4, 0, 0, ms) == -2
    assert L.drs_kernel_solve_fix(kvc.h, 1, 2, None, 4, 5, 1e-3, 8, 1, 0, None, None) == -2

    def ops(src=None, res=None, fix=None, scale=None, coef=None, size=None):
        return ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands) if size is None else size, src, res, fix, scale, coef))

    def every(k, o, want=-2):
        assert L.drs_kernel_launch_ops(k.h, 1, 2, o, 0) == want and L.drs_kernel_run_ops(k.h, 1, 2, o, 4, 0, 0) == want
        assert L.drs_kernel_run_timed_ops(k.h, 1, 2, o, 4, 0, 0, ms) == want
        assert L.drs_kernel_solve_ops(k.h, 1, 2, o, 1e-3, 8, 1, 0, None, None) == want
    # coef missing on a --varcoef kernel, coef set on every old kind of kernel, the older and shorter block, a longer one
    every(kvc, ops())
    assert L.drs_kernel_launch_gold_ops(kvc.h, 1, 2, ops(), 0) == -2
    for k, good in ((kplain, {}), (ksrc, {"src": 3}), (kfix, {"fix": 5}), (kres, {"res": 4}), (kscl, {"scale": 6})):
        every(k, ops(coef=7, **good))
        assert L.drs_kernel_launch_gold_ops(k.h, 1, 2, ops(coef=7, **{n: v for n, v in good.items() if n != "res"}), 0) == -2
    for name, v in (("src", 3), ("res", 4), ("fix", 5), ("scale", 6)):
        every(kvc, ops(coef=7, **{name: v}))
    for size in (ctypes.sizeof(drs.Operands) - 8, ctypes.sizeof(drs.Operands) + 8, 8, 0):
        every(kvc, ops(coef=7, size=size))
        every(kplain, ops(size=size))
    assert L.drs_kernel_solve_ops(kvc.h, 1, 2, ops(coef=7), 1e-3, 8, 1, 0, None, None) == -2          # a good block, but no --residual max
    # positional construction with five values keeps working
    o5 = drs.Operands(ctypes.sizeof(drs.Operands), 3, 4, 5, 6)
    assert o5.scale == 6 and o5.coef is None
    # Python: the argument checks of d_coef are those of d_fix
    for call in (kvc.launch, kvc.launch_gold, kvc.run, kvc.run_timed):
        with pytest.raises(ValueError, match="needs d_coef"):
            call(1, 2)
    for call in (kplain.launch, kplain.launch_gold, kplain.run, kplain.run_timed, kscl.launch):
        with pytest.raises(ValueError, match="without --varcoef"):
            call(1, 2, d_coef=3, **({"d_scale": 6} if call == kscl.launch else {}))
    with pytest.raises(ValueError):
        kvc.solve(1, 2, None, 1e-3, 8, d_coef=5)
    with pytest.raises(ValueError, match="without --varcoef"):
        kplain.solve(1, 2, None, 1e-3, 8, d_coef=5)
    with pytest.raises(ValueError, match="without --source"):
        kvc.launch(1, 2, d_coef=5, d_src=3)
    with pytest.raises(ValueError, match="without --scale"):
        kvc.launch(1, 2, d_coef=5, d_scale=3)


# ---- bit-exactness --------------------------------------------------------------------------------------------------------------------
_EXACT = vc.CASES + vc.MODES


@pytest.mark.parametrize("cid,ndim,src,opts", _EXACT, ids=[c[0] for c in _EXACT])
def test_emulated_varcoef_cases(tmp_path, monkeypatch, cid, ndim, src, opts):
    stc = _case_stc(tmp_path, cid, ndim, src)
    full = vc.with_vc(opts)
    lib = vc.build_emulated(tmp_path, stc, full)
    spec = oracle.Spec(stc, ndim, 1)
    assert lib.info["varcoef"] == 1 and lib.info["stages"] == 1 and lib.info["coef_taps"] == [list(o) for o, _ in spec.points]
    if cid.startswith(vc.BIG[0]):
        i = lib.info          # 16 x 4 lanes, 9 stream blocks of 54 tiles, and more launched workgroups than tiles: some leave at once
        assert i["threads"] == 64 and i["stream_blocks"] == 9 and i["tiles_x"] * i["tiles_y"] == 54 and i["grid"] == 488 > 486
    A0, B0, F0, X, W, K = vc.inputs(spec, full)
    ki = np.stack([rc.interior(k, spec.halo) for k in K])
    assert ki[0].size == 1 or ((ki < 0).any(axis=tuple(range(1, ki.ndim))).all() and (np.abs(ki) > 1).any(axis=tuple(range(1, ki.ndim))).all())
    assert len({k.tobytes() for k in K}) == len(K)                          # on the inputs alone: every tap's grid is its own
    _both_orders_and_gold(lib, tmp_path, monkeypatch, spec, ndim, full, A0, B0, F0, X, W, K, cid)


# ---- constant arrays change nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", vc.UNCHANGED, ids=[c[0] for c in vc.UNCHANGED])
def test_emulated_constant_arrays_equal_the_plain_command(tmp_path, cid, ndim, src, opts):
    """a_t[p] = (real_t)(c_t) everywhere: the stored bits are those of the same command without the option, which pins the feature to
    oracle.sweep(contract=1)."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    with_opt = vc.build_emulated(tmp_path, stc, vc.with_vc(opts))
    plain = vc.build_emulated(tmp_path, stc, list(opts))
    assert not plain.varcoef and "varcoef" not in plain.info
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W, _ = vc.inputs(spec, opts)
    K = vc.constant_coefficients(spec, A0.dtype)
    A1, B1, A2, B2, A3, B3 = A0.copy(), B0.copy(), A0.copy(), B0.copy(), A0.copy(), B0.copy()
    for t in range(2):
        a, b = ((A1, B1), (B1, A1))[t]
        assert with_opt.launch(a, b, F0, None, None, None, K) == 0
        a, b = ((A2, B2), (B2, A2))[t]
        assert plain.launch(a, b, F0) == 0
        assert bit_equal(A1, A2) and bit_equal(B1, B2), (cid, t)
        if F0 is None and "--time-order" not in opts:
            a, b = ((A3, B3), (B3, A3))[t]
            oracle.sweep(spec, a, b, contract=1)
            assert bit_equal(A1, A3) and bit_equal(B1, B3), (cid, t, "oracle")


# ---- exact integers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", vc.INTEGER, ids=[c[0] for c in vc.INTEGER])
def test_emulated_exact_integers(tmp_path, cid, ndim, src, opts):
    """in in [-4, 4], a_t[p] = ((7 t + hash(p)) mod 7) - 3: every product and sum is exact, and plain integer numpy is the reference."""
    stc = shutil.copy(src, str(tmp_path))
    lib = vc.build_emulated(tmp_path, stc, vc.with_vc(opts))
    spec = oracle.Spec(stc, ndim, 1)
    A, K, want = vc.integer_problem(spec, np.dtype(vc.dtype_of(opts)))
    assert len({k.tobytes() for k in K}) == len(K) and np.abs(want).max() > 8
    for gold in (False, True):
        B = np.full(A.shape, 0.5, A.dtype)
        assert (lib.gold(A, B, None, None, None, K) if gold else lib.launch(A, B, None, None, None, None, K)) == 0
        got = rc.interior(B, spec.halo)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(A.dtype)), (cid, gold, int((got != want).sum()))
        assert (B[ring_mask(spec.shape, spec.halo)] == 0.5).all()


# ---- tap identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", vc.IDENTITY, ids=[c[0] for c in vc.IDENTITY])
def test_emulated_tap_identity(tmp_path, cid, ndim, src, opts):
    """Coefficients zero everywhere except one tap's grid at one cell, for every tap in turn, at a corner cell, a seam cell and an interior
    cell: exactly that cell differs from zero, by exactly a * in[p + d_t]."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    lib = vc.build_emulated(tmp_path, stc, vc.with_vc(opts))
    spec = oracle.Spec(stc, ndim, 1)
    A = vc.inputs(spec, opts)[0]
    assert (A != 0).all()
    taps = vc.taps_of(spec)
    a = np.asarray(1.25, A.dtype)
    for cell in vc.identity_cells(lib.info, A.shape):
        for t, d in enumerate(taps):
            K = np.zeros((len(taps),) + A.shape, A.dtype)
            K[t][cell] = a
            B = np.full(A.shape, 0.5, A.dtype)
            assert lib.launch(A, B, None, None, None, None, K) == 0
            want = np.zeros(A.shape, A.dtype)
            want[ring_mask(spec.shape, spec.halo)] = 0.5
            want[cell] = a * A[tuple(c + o for c, o in zip(cell, d))]
            assert want[cell] != 0 and np.array_equal(B, want), (cid, cell, t, np.argwhere(B != want)[:4])


# ---- special values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("held", [False, True], ids=["free", "dirichlet"])
@pytest.mark.parametrize("cid,ndim,src,opts", vc.SPECIAL, ids=[c[0] for c in vc.SPECIAL])
def test_emulated_special_values(tmp_path, cid, ndim, src, opts, held):
    stc = shutil.copy(src, str(tmp_path))
    full = vc.with_vc(list(opts) + (vc.DIR if held else []))
    lib = vc.build_emulated(tmp_path, stc, full)
    spec = oracle.Spec(stc, ndim, 1)
    A0, B0, F0, X, W, K, p, q = vc.special_problem(spec, full, lib.info, held)
    # on the reference alone: the inf reaches its neighbours (inf or NaN there), the -0.0 block gives a zero, every special is in the interior
    Br = B0.copy()
    vc.host_launch(spec, ndim, full, A0.copy(), Br, F0, X, W, K)
    assert not np.isfinite(Br[p]) or held
    assert Br[p] == 0.5 if held else True
    assert Br[q] == 0
    assert (~np.isfinite(rc.interior(Br, spec.halo))).sum() >= 3
    ki = np.stack([rc.interior(k, spec.halo) for k in K])
    for v in sc.w_specials(A0.dtype):
        assert (np.isnan(ki).any() if np.isnan(v) else (ki.view(np.uint32 if ki.itemsize == 4 else np.uint64) == np.asarray(v).view(np.uint32 if ki.itemsize == 4 else np.uint64)).any()), v
    for gold in (False, True):
        _launches(lib, spec, ndim, full, A0, B0, F0, X, W, K, (cid, held, gold), launches=2, gold=gold)


# ---- memory contract and read log -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", vc.CONTRACT, ids=[c[0] for c in vc.CONTRACT])
def test_varcoef_memory_contract(tmp_path, cid, ndim, src, opts):
    """in, out, src, coef (and d_res) each flush against PROT_NONE pages (end-flush and start-flush), in a child process: no SIGSEGV, exact
    arrays, out's ring unchanged, coef unwritten and the NaN ring of every coefficient grid without effect."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    for o in (vc.with_vc(opts), vc.with_vc(list(opts) + vc.SOURCE + rc.RES)):
        lib = vc.build_emulated(tmp_path, stc, o)
        job = {"so": lib.so, "stc": stc, "ndim": ndim, "opts": o, "placements": ["end", "start"]}
        jpath = str(tmp_path / "job.json")
        with open(jpath, "w") as f:
            json.dump(job, f)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "varcoef_child.py"), jpath], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (o, p.returncode, p.stdout[-1500:], p.stderr[-1500:])


@pytest.mark.parametrize("cid,ndim,src,opts", vc.READLOG, ids=[c[0] for c in vc.READLOG])
def test_varcoef_read_log(tmp_path, cid, ndim, src, opts):
    """With tests/source_readlog.h in front and the watch laid over coef, one launch reads every interior byte of every grid and no ring byte."""
    stc = _case_stc(tmp_path, cid, ndim, src)
    full = vc.with_vc(opts)
    lib = vc.build_emulated(tmp_path, stc, full, read_log=True)
    spec = oracle.Spec(stc, ndim, 1)
    A, B, F, X, W, K = vc.inputs(spec, full)
    seen = np.zeros(K.nbytes, np.uint8)
    lib.lib.drs_readlog_watch(K.ctypes.data, K.nbytes, seen.ctypes.data)
    assert lib.launch(A, B, F, None, X, W, K) == 0
    lib.lib.drs_readlog_watch(None, 0, None)
    seen = seen.reshape((len(K),) + tuple(spec.shape) + (K.itemsize,))
    ring = ring_mask(spec.shape, spec.halo)
    for t in range(len(K)):
        assert seen[t][~ring].all(), (cid, t, "interior bytes of the tap's grid not read", int((seen[t][~ring] == 0).sum()))
        assert not seen[t][ring].any(), (cid, t, "ring bytes of the tap's grid read", int(seen[t][ring].sum()))


# ---- the sample of the tuner's space --------------------------------------------------------------------------------------------------
SMALL_GRID = {3: (13, 21, 300), 2: (1, 37, 300)}       # tiny ragged grids: more than one stream block, a partial x-edge tile
_SAMPLE = list(enumerate(vc.sample_jobs()))


@pytest.mark.parametrize("n,job", _SAMPLE, ids=["%02d" % n for n, _ in _SAMPLE])
def test_emulated_varcoef_sampled_fuzz(tmp_path, monkeypatch, n, job):
    """The sample on tiny grids.  What the generator refuses there it refuses with a message: its own about --varcoef (packed pairs, a
    schedule it does not serve), or the one the same command gets without the option."""
    ndim, path, dtype, args, step = job
    opts = args[:-1]
    assert "--varcoef" in opts and step == 1
    stc = _small_stc(tmp_path, path, ndim, SMALL_GRID[ndim])
    p = _cli(opts + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
    if p.returncode != 0:
        q = _cli(vc.plain_opts(opts) + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
        assert p.returncode == 255 and (q.returncode == 255 or "--varcoef" in p.stderr), (p.stderr, q.stderr)
        return
    lib = vc.build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, step)
    A0, B0, F0, X, W, K = vc.inputs(spec, opts)
    monkeypatch.delenv("EMU_ORDER", raising=False)
    _launches(lib, spec, ndim, opts, A0, B0, F0, X, W, K, (n, "forward"))
    monkeypatch.setenv("EMU_ORDER", "reverse")
    _launches(_second_lib(lib, tmp_path, "rev"), spec, ndim, opts, A0, B0, F0, X, W, K, (n, "reverse"))


def test_varcoef_sample_size():
    jobs = vc.sample_jobs()
    assert len(jobs) == vc.SAMPLE_SIZE == 20 and jobs == vc.sample_jobs() and all("--varcoef" in j[3] and "--time-order" not in j[3] for j in jobs)
    # what the GENERATOR refuses of the sample (the compiler's refusals, spills, are decided when build() compiles; the GPU suite compares
    # the whole list): exactly the listed entries that are its decisions, each for the listed reason, and with the listed spills at most 5
    said = {n: _cli(j[3], ROOT).stderr for n, j in enumerate(jobs) if drs.generate(j[3])[0] != 0}
    listed = {n: why for n, why in vc.REFUSED if "spills" not in why}
    assert sorted(said) == sorted(listed) == [9, 12, 19], (sorted(said), sorted(listed))
    for n, why in listed.items():
        assert why.split(" (")[0].split(":")[0] in said[n], (n, why, said[n])
    assert len(vc.REFUSED) == len(said) + sum("spills" in why for _, why in vc.REFUSED) <= vc.SAMPLE_SIZE - vc.MIN_CHECKED == 5


# ---- run to tolerance -----------------------------------------------------------------------------------------------------------------
def _emulated_solve(lib, A, B, F, K, tol, max_launches, check_every):
    """drs_kernel_solve_ops' loop on an emulated plugin: the library's own loop needs a device; its decisions are these."""
    n, r = 0, None
    limit = max_launches - max_launches % 2
    res = _nan_res(lib, A.dtype)
    while n < limit:
        for _ in range(min(check_every, (limit - n) // 2)):
            assert lib.launch(A, B, F, res, None, None, K) == 0 and lib.launch(B, A, F, res, None, None, K) == 0
            n += 2
        r = res[0]
        if np.isnan(r) or np.isinf(r):
            return -4, n, r
        if r <= tol:
            return 0, n, r
    return 1, n, r


@pytest.mark.parametrize("cid,ndim,src,opts,tol", vc.SOLVE, ids=[c[0] for c in vc.SOLVE])
def test_emulated_run_to_tolerance(tmp_path, cid, ndim, src, opts, tol):
    """Jacobi for -div(kappa grad u) = 1 with a two-valued kappa (1 and 10) and a ring of 0: status, launch count, residual bits and both
    arrays equal a numpy loop of the host reference that looks at r at the same launches (check_every = 4 pairs)."""
    stc = vc.solve_stc(tmp_path, ndim, src)
    lib = vc.build_emulated(tmp_path, stc, vc.solve_opts(opts))
    spec = oracle.Spec(stc, ndim, 1)
    dt = vc.dtype_of(opts)
    A, B, F, K = vc.divgrad_problem(spec, dt)
    ki = np.stack([rc.interior(k, spec.halo) for k in K])
    assert len(np.unique(ki)) >= 4 and np.allclose(ki.sum(axis=0), 1, atol=1e-5)           # a jump: several face values; rows sum to 1
    Ar, Br = A.copy(), B.copy()
    want = vc.oracle_solve(spec, ndim, Ar, Br, F, K, tol, vc.MAX_LAUNCHES, 4)
    assert want[0] == 0 and 8 < want[1] < vc.MAX_LAUNCHES and want[1] % 8 == 0, want
    K0 = K.copy()
    got = _emulated_solve(lib, A, B, F, K, tol, vc.MAX_LAUNCHES, 4)
    print(cid, "launches", got[1], "residual", got[2])
    assert got[0] == 0 and got[1] == want[1] and rc.same_bits(got[2], want[2]), (got, want)
    assert bit_equal(A, Ar) and bit_equal(B, Br) and bit_equal(K, K0)
    assert A.min() >= 0.0 and rc.interior(A, spec.halo).max() > 0.01
