"""--time-order 2 (out = S(in) - out_old, the leapfrog update) without a GPU: the generator's option surface, emitted kernels under the
CPU emulation (tests/emu) bit for bit against the host reference of tests/wave_cases.py, the extended memory contract on arrays flush
against inaccessible pages, the cross-talk check and the analytic plane wave.  The emulated cases run the stencils of the named specs
on smaller grids (more than one tile and stream block, partial tiles), so that each takes seconds."""
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
from emu_util import DRSTENCIL, build_emulated
from gpu_cases import SMALL as GPU_SMALL
from helpers import write_stc
from wave_cases import ORDER2, PERIODIC, SMALL, host_run, interior, plane_wave, stc as stc_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = os.path.join(ROOT, "benchmarks", "configs", "c4_3d7pt_star_1024.stc")

# grids of the emulated runs, by case id: (L, M, N)
DIMS = {
    "3d_star_fp32": (19, 37, 264),                # 2 x 2 tiles of 256 x 32, 3 stream blocks of 8; N % 4 == 0: 16-byte vectors, partial x-edge tile
    "3d_star_oddN_fp64_elem": (13, 21, 135),      # N * 8 % 16 != 0: element accesses
    "3d_cross_reuse_dist2": (15, 19, 268),
    "3d_window_prefetch": (21, 19, 264),
    "3d_rows_prefetch": (21, 19, 264),
    "3d_dma_fp64": (13, 19, 140),
    "3d_store_mask_buffer": (13, 37, 264),
    "3d_defer_stores": (13, 19, 264),
    "3d_zigzag": (36, 19, 264),
    "3d_ahead_fp64": (15, 19, 140),
    "2d_star_tile_fp32": (1, 41, 268),
    "2d_box25_tile_fp64": (1, 41, 140),
    "2d_star_stream_fp32": (1, 61, 268),
    "2d_odd_stream_fp64": (1, 30, 137),
}


def _cli(args, cwd):
    return subprocess.run([DRSTENCIL] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


def _small_stc(tmp_path, src, ndim, dims, iters=4, name=None):
    """The stencil of `src` on a grid of `dims`."""
    pts = [tuple(off[3 - ndim:]) + (c,) for off, c in oracle.Spec(src, ndim, 1).points]
    path = os.path.join(str(tmp_path), (name or os.path.basename(src)[:-4]) + ".stc")
    write_stc(path, ndim, dims, iters, pts)
    return path


def _rand(shape, dt, seed):
    return np.random.default_rng(seed).random(shape).astype(dt)


def _launches(fn, A, B, n):
    for t in range(n):
        s, d = (A, B) if t % 2 == 0 else (B, A)
        assert fn(s.ctypes.data, d.ctypes.data, None) == 0


def _second_lib(lib_path, tmp_path, tag):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    import ctypes
    cp = os.path.join(str(tmp_path), tag + "_" + os.path.basename(lib_path))
    shutil.copy(lib_path, cp)
    lib = ctypes.CDLL(cp)
    for n in ("drs_plugin_launch", "drs_plugin_launch_gold"):
        getattr(lib, n).argtypes = [ctypes.c_void_p] * 3
    return lib


# ---- generator / CLI ------------------------------------------------------------------------------------------------------------------
def test_time_order_1_emits_todays_source():
    """--time-order 1 is the default spelled out: same messages, same source, byte for byte."""
    seen = 0
    for cid, ndim, stc, opts in GPU_SMALL[::7] + [("c4", 3, C4, ["--3d", "--dtype", "fp32", "--step", "2"])]:
        r0 = drs.generate(opts + [stc])
        r1 = drs.generate(opts + ["--time-order", "1", stc])
        r2 = drs.generate(["--time-order", "1"] + opts + [stc])
        assert r0 == r1 == r2, cid
        assert r0[2] is None or ("ov0_" not in r0[2] and "time_order" not in r0[2]), cid
        seen += r0[2] is not None
    assert seen >= 5


def test_cli_time_order_2(tmp_path):
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (10, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + ORDER2 + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "out_old" not in p.stdout and "time" not in p.stdout              # stdout stays the reference's protocol
    assert "drstencil: note: second-order time stepping: a launch computes out = S(in) - out_old on the interior" in p.stderr
    src = open(out).read()
    assert "// options: --3d --dtype fp32 --time-order 2" in src
    assert "] = t - d_out[" in src                                             # the gold kernel
    info = json.loads(re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', src).group(1).replace('\\"', '"'))
    assert info["time_order"] == 2
    # the C ABI's generator agrees with the command
    rc, msg, src2 = drs.generate(["--3d", "--dtype", "fp32"] + ORDER2 + ["-o", out, stc])
    assert rc == 0 and src2 == src and "second-order time stepping" in msg
    # without the option: no key, no trace
    p = _cli(["--3d", "--dtype", "fp32", "--time-order", "1", "-o", out, stc], tmp_path)
    assert p.returncode == 0 and "second-order" not in p.stderr
    src1 = "".join(ln for ln in open(out) if not ln.startswith(("// spec:", "// options:")))      # (the banner holds this test's paths)
    assert "time_order" not in src1 and "time-order" not in src1 and "ov0_" not in src1
    assert "time-order" not in [ln for ln in open(out) if ln.startswith("// options:")][0].replace(str(tmp_path), "")


def test_cli_rejects_bad_time_order(tmp_path):
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (10, 12, 16), name="p")
    for v in ("0", "3", "two"):
        p = _cli(["--3d", "--time-order", v, "-o", str(tmp_path / "k.hip"), stc], tmp_path)
        assert p.returncode == 255 and p.stdout == "Illegal input.\n", (v, p.stdout)
    p = _cli(["--3d", "--time-order", stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Illegal input.\n"


@pytest.mark.parametrize("extra,reason", [
    (["--step", "2"], "--time-order 2 needs --step 1"),
    (["--temporal", "1"], "--time-order 2 cannot be combined with --temporal"),
    (["--temporal", "force"], "--time-order 2 cannot be combined with --temporal"),
    (["--step", "2", "--temporal", "1"], "--time-order 2 needs --step 1"),
    (["--gpus", "2"], "--time-order 2 cannot be combined with --gpus N > 1"),
    (["--pair-launch", "1"], "--time-order 2 cannot be combined with --pair-launch 1"),
])
def test_cli_time_order_2_rejections(tmp_path, extra, reason):
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + ORDER2 + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", (p.returncode, p.stdout)
    assert reason in p.stderr, p.stderr
    assert not os.path.exists(out)
    # the same command line is legal with --time-order 1
    p = _cli(["--3d", "--dtype", "fp32"] + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr


def test_bare_c4_order_2_keeps_the_tuned_row():
    """--time-order names the problem: a bare C4 command line still takes the tuner's step-1 row."""
    args = ["--3d", "--dtype", "fp32"]
    rc0, msg0, src0 = drs.generate(args + [C4])
    rc1, msg1, src1 = drs.generate(args + ORDER2 + [C4])
    assert rc0 == rc1 == 0
    row = re.search(r"is used \((.*?)\)", msg0).group(1)
    assert "is used (%s)" % row in msg1
    assert "ov1_0_0" in src1 and "ov0_" not in src0
    i0, i1 = (json.loads(re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', s).group(1).replace('\\"', '"')) for s in (src0, src1))
    # the named registers of the old output: RY * VX words per set, prefetch depth + 1 sets
    assert i1["reg_demand"] == i0["reg_demand"] + i0["points_per_lane"] * 2 and "time_order" not in i0


def test_slab_forms_refuse_time_order_2(tmp_path):
    from drstencil_amd import multigpu
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (16, 12, 16), name="p")
    opts = ["--3d", "--dtype", "fp32"] + ORDER2
    with pytest.raises(ValueError, match="time-order 2"):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match="time-order 2"):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match="time-order 2"):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match="time-order 2"):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    with pytest.raises(drs.KernelBuildError, match="--time-order 2 is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))


# ---- emulated kernels against the host reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", SMALL, ids=[c[0] for c in SMALL])
def test_emulated_order_2_bit_exact(tmp_path, monkeypatch, cid, ndim, src, opts):
    """2 launches (both directions of the ping-pong) and 5 (an odd count) from random A AND random B -- with B = 0 the first launch
    cannot tell -out_old from nothing -- in both fiber orders of the emulator; the gold kernel against the same reference."""
    stc = _small_stc(tmp_path, src, ndim, DIMS[cid])
    lib = build_emulated(tmp_path, stc, opts)
    info = json.loads(lib.drs_plugin_info().decode())
    assert info["time_order"] == 2 and info["stages"] == 1
    spec = oracle.Spec(stc, ndim, 1)
    dt = np.float32 if "fp32" in opts else np.float64
    A0, B0 = _rand(spec.shape, dt, 11), _rand(spec.shape, dt, 12)
    refs = {}
    for n in (2, 5):
        Ar, Br = A0.copy(), B0.copy()
        host_run(spec, Ar, Br, n)
        refs[n] = (Ar, Br)
    assert not np.array_equal(interior(refs[2][1], spec.halo), interior(B0, spec.halo))
    # the emulator latches EMU_ORDER at a loaded object's first launch: the forward runs come first, the second copy is loaded and
    # launched with the variable set
    monkeypatch.delenv("EMU_ORDER", raising=False)
    for what, counts in (("forward", (2, 5)), ("gold", (5,)), ("reverse", (5,))):
        if what == "reverse":
            monkeypatch.setenv("EMU_ORDER", "reverse")
            fn = _second_lib(lib._name, tmp_path, "rev").drs_plugin_launch
        else:
            fn = lib.drs_plugin_launch if what == "forward" else lib.drs_plugin_launch_gold
        for n in counts:
            A, B = A0.copy(), B0.copy()
            _launches(fn, A, B, n)
            assert np.array_equal(A, refs[n][0]) and np.array_equal(B, refs[n][1]), (cid, what, n)


XTALK = [c for c in SMALL if c[0] in ("3d_star_fp32", "3d_star_oddN_fp64_elem")]


@pytest.mark.parametrize("cid,ndim,src,opts", XTALK, ids=[c[0] for c in XTALK])
def test_old_value_reaches_only_its_own_cell(tmp_path, cid, ndim, src, opts):
    """NaN in single interior cells of the old output: the result holds NaN in exactly those cells (an old value loaded from a
    neighbouring cell, row or plane would move or spread them)."""
    stc = _small_stc(tmp_path, src, ndim, DIMS[cid])
    lib = build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, 1)
    dt = np.float32 if "fp32" in opts else np.float64
    H = spec.halo
    L, M, N = spec.shape
    # a cell in the first and the last stream block, at the edges and inside the tiles' x / y ranges
    for cell in [(H, H, H), (L - H - 1, M - H - 1, N - H - 1), (L // 2, M // 2, N // 2), (H + 1, M - H - 1, 255), (9, 32, 256)]:
        cell = tuple(min(max(c, H), n - H - 1) for c, n in zip(cell, spec.shape))
        A, B = _rand(spec.shape, dt, 3), _rand(spec.shape, dt, 4)
        B[cell] = np.nan
        assert lib.drs_plugin_launch(A.ctypes.data, B.ctypes.data, None) == 0
        where = np.argwhere(np.isnan(B))
        assert where.shape[0] == 1 and tuple(where[0]) == cell, (cid, cell, where[:4])


FOOTPRINT = [c for c in SMALL if c[0] in ("3d_star_fp32", "3d_store_mask_buffer", "3d_star_oddN_fp64_elem", "2d_star_tile_fp32")]


@pytest.mark.parametrize("cid,ndim,src,opts", FOOTPRINT, ids=[c[0] for c in FOOTPRINT])
def test_order_2_memory_contract(tmp_path, cid, ndim, src, opts):
    """Both arrays flush against PROT_NONE pages (end-flush and start-flush), NaN in every unread cell of `in` and in the whole ring of
    `out`, finite data in out's interior: no NaN in out's interior, out's ring bit-unchanged, no SIGSEGV."""
    stc = _small_stc(tmp_path, src, ndim, DIMS[cid])
    lib = build_emulated(tmp_path, stc, opts)
    job = {"so": lib._name, "stc": stc, "ndim": ndim, "dtype": "float32" if "fp32" in opts else "float64", "placements": ["end", "start"]}
    jpath = str(tmp_path / "job.json")
    with open(jpath, "w") as f:
        json.dump(job, f)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wave_child.py"), jpath], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (p.returncode, p.stdout[-1500:], p.stderr[-1500:])


# ---- the analytic plane wave -----------------------------------------------------------------------------------------------------------
def test_emulated_plane_wave_fp64(tmp_path):
    """t3_wave, periodic, fp64: A = cos(k.x), B = cos(k.x + w) with k = 2 pi (1/20, 2/24, 3/128) over the period and
    cos w = (c0 + 2 lambda sum cos k_d) / 2.  u(t) = cos(k.x - w t) solves the leapfrog recurrence exactly, so after the spec's 8
    launches the array written last equals cos(k.x - 8 w) up to rounding: 1e-12, the project's fp64 bar (numpy gives 7e-15)."""
    src = stc_path("t3_wave")
    lib = build_emulated(tmp_path, src, ["--3d", "--dtype", "fp64", "--sn", "8"] + PERIODIC + ORDER2)
    spec = oracle.Spec(src, 3, 1)
    assert spec.shape == (22, 26, 130) and spec.halo == 1 and spec.launches == 8
    A, B, exact = plane_wave(spec.shape, 1, spec.points)
    _launches(lib.drs_plugin_launch, A, B, 8)
    err = np.max(np.abs(interior(A, 1) - exact(8)))          # odd launches write B, even ones A
    print("plane wave after 8 launches: max abs error %.3g" % err)
    assert err <= 1e-12, err
    assert np.max(np.abs(interior(B, 1) - exact(7))) <= 1e-12
