"""--boundary periodic without a GPU: the generator's option surface, the emitted wrap kernel and whole periodic runs of emitted
kernels under the CPU emulation (tests/emu), against the CPU oracle with the ring filled from the interior before every launch and
against an oracle-free np.roll reference; the slab runtime's refusals."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import drstencil_amd as drs
import oracle
from emu_util import DRSTENCIL, build_emulated, run_emulated
from gpu_cases import SMALL as GPU_SMALL
from helpers import write_stc
from periodic_cases import PERIODIC, host_wrap, oracle_periodic_run, roll_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = os.path.join(ROOT, "benchmarks", "configs", "c4_3d7pt_star_1024.stc")

# one-step stencils with short decimal coefficients (the fused stencils' coefficients stay exact at the 6 significant digits the
# generator prints, so fused step n and n np.roll steps agree to rounding) and no symmetry (a mirrored wrap would show)
STAR3 = [(0, 0, 0, 0.25), (1, 0, 0, 0.1), (-1, 0, 0, 0.15), (0, 1, 0, 0.12), (0, -1, 0, 0.13), (0, 0, 1, 0.11), (0, 0, -1, 0.14)]
CROSS3 = STAR3 + [(2, 0, 0, 0.01), (0, -2, 0, 0.02)]
STAR2 = [(0, 0, 0.3), (1, 0, 0.1), (-1, 0, 0.2), (0, 1, 0.15), (0, -1, 0.25)]
BOX9 = [(j, i, 0.1 + 0.01 * (3 * (j + 1) + i + 1)) for j in (-1, 0, 1) for i in (-1, 0, 1)]
SHAPES = {"STAR3": (3, STAR3), "CROSS3": (3, CROSS3), "STAR2": (2, STAR2), "BOX9": (2, BOX9)}


def _stc(tmp_path, shape, dims, iters=4, name="p"):
    ndim, pts = SHAPES[shape]
    path = os.path.join(str(tmp_path), "%s.stc" % name)
    write_stc(path, ndim, dims, iters, pts)
    return path


def _cli(args, cwd):
    return subprocess.run([DRSTENCIL] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


def _interior(a, H):
    return a[tuple(slice(H, n - H) for n in a.shape)]


def _fill(shape, dtype, seed=7):
    return np.random.default_rng(seed).random(shape).astype(dtype)


# ---- generator / CLI ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim,dtype", [(3, "fp32"), (3, "fp64"), (2, "fp32"), (2, "fp64")])
def test_cli_accepts_periodic(tmp_path, ndim, dtype):
    stc = _stc(tmp_path, "STAR3" if ndim == 3 else "STAR2", (10, 12, 16) if ndim == 3 else (1, 12, 16))
    out = str(tmp_path / "k.hip")
    p = _cli((["--3d"] if ndim == 3 else []) + ["--dtype", dtype, "--step", "2"] + PERIODIC + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "periodic" not in p.stdout                            # stdout stays the reference's protocol
    per = "6 x 8 x 12" if ndim == 3 else "8 x 12"                # period = dim - 2 Halo, Halo = step * order = 2
    assert "drstencil: note: periodic boundaries: period %s, ring of width 2 holds ghost copies" % per in p.stderr, p.stderr
    src = open(out).read()
    assert "__global__ void __launch_bounds__(256) wrap_p (real_t* __restrict__ a)" in src
    assert 'extern "C" int drs_plugin_wrap(void* a, hipStream_t stream)' in src
    # both launch entry points wrap their input first
    for ep in ("drs_plugin_launch", "drs_plugin_launch_gold"):
        body = src[src.index('extern "C" int %s(' % ep):]
        assert body.split("\n")[2].strip().startswith("if (int rc = drs_plugin_wrap((void*)in, stream)) return rc;"), ep
    info = re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', src).group(1).replace('\\"', '"')
    assert ('"boundary":"periodic","period":[6,8,12]' if ndim == 3 else '"boundary":"periodic","period":[8,12]') in info


def test_cli_rejects_bad_boundary(tmp_path):
    stc = _stc(tmp_path, "STAR3", (10, 12, 16))
    for v in ("torus", "Periodic", ""):
        p = _cli(["--3d", "--boundary", v, "-o", str(tmp_path / "k.hip"), stc], tmp_path)
        assert p.returncode == 255 and p.stdout == "Illegal input.\n", (v, p.stdout)
    # a value-taking flag in the second-to-last slot (main.cpp's scan)
    p = _cli(["--3d", "--boundary", stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Illegal input.\n"


@pytest.mark.parametrize("dims,step", [((10, 12, 5), 2), ((5, 12, 16), 2), ((10, 5, 16), 2)])
def test_cli_periodic_needs_three_halos(tmp_path, dims, step):
    stc = _stc(tmp_path, "STAR3", dims)
    p = _cli(["--3d", "--dtype", "fp32", "--step", str(step)] + PERIODIC + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", p.stdout
    assert "3 * Halo" in p.stderr
    # the same grid is legal with a fixed ring
    p = _cli(["--3d", "--dtype", "fp32", "--step", str(step), "-o", str(tmp_path / "k.hip"), stc], tmp_path)
    assert p.returncode == 0, p.stdout


@pytest.mark.parametrize("extra,what", [(["--gpus", "2"], "--gpus N > 1"), (["--pair-launch", "1"], "--pair-launch 1")])
def test_cli_periodic_refuses_slab_forms(tmp_path, extra, what):
    stc = _stc(tmp_path, "STAR3", (16, 12, 16))
    p = _cli(["--3d", "--dtype", "fp32"] + PERIODIC + extra + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n"
    assert "--boundary periodic cannot be combined with " + what in p.stderr, p.stderr
    assert not os.path.exists(str(tmp_path / "k.hip"))


def test_boundary_fixed_emits_todays_source():
    """--boundary fixed is the default spelled out: the emitted source is byte for byte that of the same command line without it."""
    seen = 0
    for cid, ndim, stc, opts in GPU_SMALL:
        rc0, msg0, src0 = drs.generate(opts + [stc])
        rc1, msg1, src1 = drs.generate(opts + ["--boundary", "fixed", stc])
        rc2, msg2, src2 = drs.generate(["--boundary", "fixed"] + opts + [stc])
        assert (rc0, msg0, src0) == (rc1, msg1, src1) == (rc2, msg2, src2), cid
        assert src0 is None or "wrap_" not in src0, cid
        seen += src0 is not None
    assert seen > 100


def test_bare_c4_periodic_keeps_the_tuned_row():
    """--boundary names the problem: a bare C4 command line still takes the tuner's row, and its sweep kernel is the fixed one."""
    args = ["--3d", "--dtype", "fp32", "--step", "2"]
    rc0, msg0, src0 = drs.generate(args + [C4])
    rc1, msg1, src1 = drs.generate(args + PERIODIC + [C4])
    assert rc0 == rc1 == 0
    assert "the tuner's configuration" in msg0 and "the tuner's configuration" in msg1, msg1
    row = re.search(r"is used \((.*?)\)", msg0).group(1)
    assert "is used (%s)" % row in msg1
    assert "periodic boundaries: period 1020 x 1020 x 1020, ring of width 2" in msg1

    def sweep_part(src):   # header and dr_ kernel: everything between the banner and the gold kernel
        return src[src.index("#include"):src.index("// naive reference kernel")]
    assert sweep_part(src0) == sweep_part(src1)
    assert "wrap_c4_3d7pt_star_1024" in src1 and "wrap_" not in src0


# ---- the wrap kernel under the emulation ------------------------------------------------------------------------------------------
def _emulated(tmp_path, stc, opts):
    lib = build_emulated(tmp_path, stc, opts)
    lib.drs_plugin_wrap.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return lib


WRAP_CASES = [
    # (id, shape, dims, options): 16-byte vector path (N * sizeof % 16 == 0) and element path, both dtypes, 2D and 3D
    ("3d_fp32_vec", "STAR3", (9, 11, 24), ["--3d", "--dtype", "fp32"]),
    ("3d_fp64_vec_step2", "STAR3", (10, 11, 14), ["--3d", "--dtype", "fp64", "--step", "2"]),
    ("3d_fp32_oddN_elem", "STAR3", (9, 11, 13), ["--3d", "--dtype", "fp32"]),
    ("3d_fp64_oddN_elem_step2", "STAR3", (8, 13, 15), ["--3d", "--dtype", "fp64", "--step", "2"]),
    ("2d_fp32_vec", "STAR2", (1, 13, 24), ["--dtype", "fp32"]),
    ("2d_fp64_elem_step3", "STAR2", (1, 17, 19), ["--dtype", "fp64", "--step", "3"]),
    ("2d_fp32_stream_vec", "BOX9", (1, 9, 36), ["--dtype", "fp32", "--streaming"]),
    # minimum legal grids: dim = 3 Halo (period = Halo)
    ("3d_min_fp32_elem", "STAR3", (3, 3, 3), ["--3d", "--dtype", "fp32"]),
    ("3d_min_fp64_vec_step2", "STAR3", (6, 6, 6), ["--3d", "--dtype", "fp64", "--step", "2"]),
    ("2d_min_fp32_vec_step4", "STAR2", (1, 12, 12), ["--dtype", "fp32", "--step", "4"]),
]


@pytest.mark.parametrize("cid,shape,dims,opts", WRAP_CASES, ids=[c[0] for c in WRAP_CASES])
def test_emulated_wrap_equals_np_pad(tmp_path, cid, shape, dims, opts):
    stc = _stc(tmp_path, shape, dims)
    lib = _emulated(tmp_path, stc, opts + PERIODIC)
    info = json.loads(lib.drs_plugin_info().decode())
    H = info["halo"]
    a0 = _fill(dims if "--3d" in opts else dims[1:], np.float32 if "fp32" in opts else np.float64)
    a = a0.copy()
    assert lib.drs_plugin_wrap(a.ctypes.data, None) == 0
    ref = np.pad(_interior(a0, H), H, mode="wrap")
    assert np.array_equal(a, ref), cid
    assert np.array_equal(host_wrap(a0.copy(), H), ref)        # the tests' host wrap is the same function


@pytest.mark.parametrize("name", ["gold_odd3d_s1", "gold_odd3d_s2", "gold_odd2d_s1", "gold_odd2d_s2"])
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_emulated_wrap_asymmetric_stencils(tmp_path, name, dtype):
    """Asymmetric stencils: Halo comes from the outermost dimension's order, the ring is Halo wide in every dimension."""
    stc = os.path.join(ROOT, "tests", "stc", name + ".stc")
    ndim = 3 if "3d" in name else 2
    step = int(name[-1])
    lib = _emulated(tmp_path, stc, (["--3d"] if ndim == 3 else []) + ["--dtype", dtype, "--step", str(step)] + PERIODIC)
    H = oracle.Spec(stc, ndim, step).halo
    a0 = _fill(oracle.Spec(stc, ndim, step).shape, np.float32 if dtype == "fp32" else np.float64, seed=3)
    a = a0.copy()
    assert lib.drs_plugin_wrap(a.ctypes.data, None) == 0
    assert np.array_equal(a, np.pad(_interior(a0, H), H, mode="wrap"))


# ---- whole periodic runs under the emulation ----------------------------------------------------------------------------------------
RUNS = [
    ("3d_step1", "STAR3", (12, 17, 264), ["--3d", "--dtype", "fp32", "--sn", "8"]),
    ("3d_fused_step2", "STAR3", (17, 21, 300), ["--3d", "--dtype", "fp32", "--sn", "6", "--step", "2", "--prefetch", "--xrim", "dpp"]),
    ("3d_fused_step3_rows", "STAR3", (19, 23, 260), ["--3d", "--dtype", "fp32", "--sn", "8", "--step", "3", "--prefetch", "--prefetch-depth", "2",
                                                     "--order", "rows", "--bx", "32", "--by", "4", "--block-merge-y", "2"]),
    ("2d_tile", "BOX9", (1, 41, 70), ["--dtype", "fp64"]),
    ("2d_streaming_step2", "STAR2", (1, 61, 268), ["--dtype", "fp32", "--streaming", "--sn", "9", "--step", "2", "--prefetch"]),
    ("3d_reuse_dist2", "CROSS3", (14, 19, 136), ["--3d", "--dtype", "fp64", "--dist", "2", "--step", "2", "--xrim", "dpp"]),
    ("3d_order_rows_fp64", "STAR3", (15, 19, 140), ["--3d", "--dtype", "fp64", "--sn", "5", "--step", "2", "--order", "rows"]),
    ("3d_temporal3_skew_fp64", "STAR3", (15, 19, 140), ["--3d", "--dtype", "fp64", "--sn", "4", "--step", "3", "--temporal", "1", "--skew", "1", "--prefetch",
                                                        "--order", "rows", "--exact-y", "1", "--bx", "34", "--by", "8", "--block-merge-y", "2"]),
]


@pytest.mark.parametrize("cid,shape,dims,opts", RUNS, ids=[c[0] for c in RUNS])
def test_emulated_periodic_run_vs_oracle_with_wrap(tmp_path, cid, shape, dims, opts):
    ndim = 3 if "--3d" in opts else 2
    step = int(opts[opts.index("--step") + 1]) if "--step" in opts else 1
    stc = _stc(tmp_path, shape, dims, iters=2 * step)             # two launches: both directions of the ping-pong
    lib = _emulated(tmp_path, stc, opts + PERIODIC)
    info = json.loads(lib.drs_plugin_info().decode())
    temporal = info["stages"] > 1
    assert temporal == ("--temporal" in opts), info
    spec = oracle.Spec(stc, ndim, step)
    dt = np.float32 if "fp32" in opts else np.float64
    A0 = _fill(spec.shape, dt, seed=11)
    B0 = _fill(spec.shape, dt, seed=12)                          # B's ring holds garbage that no periodic launch may read
    A, B = A0.copy(), B0.copy()
    n = run_emulated(lib, A, B, spec.iterations, step)
    Ar, Br = A0.copy(), B0.copy()
    assert oracle_periodic_run(spec, Ar, Br) == n == 2
    if temporal:
        for got, ref in ((A, Ar), (B, Br)):
            rel = np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-30))
            assert rel <= (1e-6 if dt == np.float32 else 1e-12), (cid, rel)
        # the rings: A's was filled from A0's interior (exact), B's from the first launch's output (within the tolerance, like it)
        H = spec.halo
        ring = np.ones(A.shape, bool)
        ring[tuple(slice(H, s - H) for s in A.shape)] = False
        assert np.array_equal(A[ring], Ar[ring])
        assert np.array_equal(B, host_wrap(B.copy(), H))
    else:
        assert np.array_equal(A, Ar) and np.array_equal(B, Br), cid
    # the gold entry point wraps too: --check and Kernel.run(gold=True) compare periodic with periodic
    Ag, Bg = A0.copy(), B0.copy()
    run_emulated(lib, Ag, Bg, spec.iterations, step, gold=True)
    assert np.array_equal(Ag, Ar) and np.array_equal(Bg, Br), cid


def test_emulated_fused_step2_equals_two_roll_steps(tmp_path):
    """Semantics, oracle-free: one fused step-2 periodic launch (fp64) == two periodic one-step updates by np.roll over the period."""
    dims = (10, 12, 14)
    stc = _stc(tmp_path, "STAR3", dims, iters=4)
    lib = _emulated(tmp_path, stc, ["--3d", "--dtype", "fp64", "--step", "2"] + PERIODIC)
    H = 2
    A0 = _fill(dims, np.float64, seed=5)
    A, B = A0.copy(), np.zeros_like(A0)
    assert run_emulated(lib, A, B, 4, 2) == 2
    pts = [((k, j, i), c) for k, j, i, c in STAR3]
    ref1 = roll_reference(pts, _interior(A0, H), 2)
    ref2 = roll_reference(pts, ref1, 2)
    for got, ref in ((_interior(B, H), ref1), (_interior(A, H), ref2)):
        rel = np.max(np.abs(got - ref) / np.abs(ref))
        assert rel <= 1e-12, rel


# ---- the slab runtime refuses periodic args ---------------------------------------------------------------------------------------
def test_multigpu_refuses_periodic(tmp_path):
    from drstencil_amd import multigpu
    stc = _stc(tmp_path, "STAR3", (16, 12, 16))
    opts = ["--3d", "--dtype", "fp32"] + PERIODIC
    with pytest.raises(ValueError, match="periodic"):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match="periodic"):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:      # a sweep that carries periodic generator options
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match="periodic"):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match="periodic"):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    # the C ABI's slab runtime: NULL + a log line naming the combination, before any kernel is built
    with pytest.raises(drs.KernelBuildError, match="--boundary periodic is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))
