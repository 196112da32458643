"""--source (out = S(in) + src; with --time-order 2 (S(in) - out_old) + src) without a GPU: the generator's option surface, emitted
kernels under the CPU emulation (tests/emu) bit for bit against the host reference of tests/source_cases.py, cross-talk, the memory
contract on three arrays flush against inaccessible pages, a manufactured fixed point and two samples of the tuner's space.  The emulated
cases run the stencils of the named specs on smaller grids (more than one tile and stream block, partial tiles), so that each takes
seconds.

Tried once by hand, not as a test: with the `scol` guards of the source stream's element loads removed from the emitter (the partial
vector's and the element-wide row's), test_source_ring_is_not_read FAILS in all nine cases (ring cells of src read at x = 0 and
x = N - 1), while test_source_memory_contract fails on edge3_thin alone and passes its other cases: most of the unguarded loads fetch
cells in the same row of src, inside the array, into registers that reach no store, which values and page protection cannot see and the
read log can."""
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
from emu_util import DRSTENCIL
from gpu_cases import SMALL as GPU_SMALL
from helpers import write_stc
from source_cases import (BOTH, CHANNEL, EMU_REFUSED, FIXED_POINT, MIN_CHECKED, ORDER2, PERIODIC, SAMPLES, SMALL, SOURCE, build_emulated, fixed_point, host_run,
                          interior, load_emulated, modes_of, sample_jobs, signed_random, stc as stc_path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = os.path.join(ROOT, "benchmarks", "configs", "c4_3d7pt_star_1024.stc")

# grids of the emulated runs, by case id (tests/test_time_order_cpu.py's): (L, M, N)
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
ALL = SMALL + BOTH


def _dims(cid):
    return DIMS[cid[:-len("_order2")] if cid.endswith("_order2") else cid]


def _cli(args, cwd):
    return subprocess.run([DRSTENCIL] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


def _small_stc(tmp_path, src, ndim, dims, iters=4, name=None):
    """The stencil of `src` on a grid of `dims`."""
    pts = [tuple(off[3 - ndim:]) + (c,) for off, c in oracle.Spec(src, ndim, 1).points]
    path = os.path.join(str(tmp_path), (name or os.path.basename(src)[:-4]) + ".stc")
    write_stc(path, ndim, dims, iters, pts)
    return path


def _dt(opts):
    return np.float32 if "fp32" in opts else np.float64


def _inputs(spec, dt):
    """Random A, B and F in [-1, 1): with F = 0 a kernel that drops the term passes."""
    return signed_random(spec.shape, dt, 11), signed_random(spec.shape, dt, 12), signed_random(spec.shape, dt, 13)


def _launches(fn, A, B, F, n):
    for t in range(n):
        s, d = (A, B) if t % 2 == 0 else (B, A)
        assert fn(s.ctypes.data, d.ctypes.data, F.ctypes.data, None) == 0


def _second_lib(lib, tmp_path, tag):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    cp = os.path.join(str(tmp_path), tag + "_" + os.path.basename(lib._name))
    shutil.copy(lib._name, cp)
    return load_emulated(cp)


def _info(src):
    return json.loads(re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', src).group(1).replace('\\"', '"'))


def _check_bit_exact(lib, spec, opts, ndim, tmp_path, monkeypatch, counts=(2, 5), gold_counts=(5,), reverse_counts=(5,)):
    """dr in both fiber orders of the emulator and gold against the host reference, all three arrays bit for bit."""
    dt = _dt(opts)
    order2 = "--time-order" in opts
    modes = modes_of(opts, ndim)
    A0, B0, F0 = _inputs(spec, dt)
    refs = {}
    for n in sorted(set(counts) | set(gold_counts) | set(reverse_counts)):
        Ar, Br = A0.copy(), B0.copy()
        host_run(spec, Ar, Br, F0, n, modes, order2)
        refs[n] = (Ar, Br)
    # the term is seen: the same run without it differs
    Az, Bz = A0.copy(), B0.copy()
    host_run(spec, Az, Bz, np.zeros_like(F0), min(refs), modes, order2)
    assert not np.array_equal(interior(Bz, spec.halo), interior(refs[min(refs)][1], spec.halo))
    # the emulator latches EMU_ORDER at a loaded object's first launch: the forward runs come first, then a second copy of the plugin
    monkeypatch.delenv("EMU_ORDER", raising=False)
    for what, cs in (("forward", counts), ("gold", gold_counts), ("reverse", reverse_counts)):
        if what == "reverse":
            monkeypatch.setenv("EMU_ORDER", "reverse")
            fn = _second_lib(lib, tmp_path, "rev").drs_plugin_launch_src
        else:
            fn = lib.drs_plugin_launch_src if what == "forward" else lib.drs_plugin_launch_gold_src
        for n in cs:
            A, B, F = A0.copy(), B0.copy(), F0.copy()
            _launches(fn, A, B, F, n)
            assert np.array_equal(F, F0), (what, n)
            assert np.array_equal(A, refs[n][0]) and np.array_equal(B, refs[n][1]), (what, n, int((A != refs[n][0]).sum()), int((B != refs[n][1]).sum()))


# ---- generator / CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_source(tmp_path):
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (10, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + SOURCE + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "src" not in p.stdout and "source" not in p.stdout                 # stdout stays the reference's protocol
    notes = [ln for ln in p.stderr.splitlines() if "source term" in ln]
    assert notes == ["drstencil: note: source term: a launch takes a third array and computes out = S(in) + src on the interior (src is read only, in its interior)"]
    src = open(out).read()
    assert "// options: --3d --dtype fp32 --source" in src
    assert "const real_t* __restrict__ d_in, real_t* __restrict__ d_out, const real_t* __restrict__ d_src)" in src
    assert "] = t + d_src[" in src and "t = t - d_out[" not in src           # the gold kernel's statements
    assert "drs_plugin_launch_src(const void* in, void* out, const void* src, hipStream_t stream)" in src
    assert "drs_plugin_launch_gold_src(" in src and "drs_plugin_launch(" not in src and "drs_plugin_launch_gold(" not in src
    info = _info(src)
    assert info["source"] == 1 and "time_order" not in info
    # the C ABI's generator agrees with the command
    rc, msg, src2 = drs.generate(["--3d", "--dtype", "fp32"] + SOURCE + ["-o", out, stc])
    assert rc == 0 and src2 == src and "drstencil: note: source term" in msg
    # with --time-order 2: three statements, in this order
    p = _cli(["--3d", "--dtype", "fp32"] + ORDER2 + SOURCE + ["-o", out, stc], tmp_path)
    assert p.returncode == 0 and "out = (S(in) - out_old) + src" in p.stderr
    src = open(out).read()
    assert src.index("t = t - d_out[") < src.index("] = t + d_src[")
    assert _info(src)["source"] == 1 and _info(src)["time_order"] == 2
    # a ring fill goes to `in` only
    p = _cli(["--3d", "--dtype", "fp32"] + CHANNEL + SOURCE + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stderr
    src = open(out).read()
    assert src.count("drs_plugin_wrap((void*)in, stream)") == 2 and "drs_plugin_wrap((void*)src" not in src


@pytest.mark.parametrize("extra,reason", [
    (["--step", "2"], "--source needs --step 1"),
    (["--temporal", "1"], "--source cannot be combined with --temporal"),
    (["--temporal", "force"], "--source cannot be combined with --temporal"),
    (["--step", "2", "--temporal", "1"], "--source needs --step 1"),
    (["--gpus", "2"], "--source cannot be combined with --gpus N > 1"),
    (["--pair-launch", "1"], "--source cannot be combined with --pair-launch 1"),
])
def test_cli_source_rejections(tmp_path, extra, reason):
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (16, 12, 16), name="p")
    out = str(tmp_path / "k.hip")
    p = _cli(["--3d", "--dtype", "fp32"] + SOURCE + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", (p.returncode, p.stdout)
    assert reason in p.stderr, p.stderr
    assert not os.path.exists(out)
    # the same command line is legal without --source
    p = _cli(["--3d", "--dtype", "fp32"] + extra + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr


def test_slab_forms_refuse_source(tmp_path):
    from drstencil_amd import multigpu
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (16, 12, 16), name="p")
    opts = ["--3d", "--dtype", "fp32"] + SOURCE
    with pytest.raises(ValueError, match="--source"):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match="--source"):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match="--source"):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match="--source"):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    with pytest.raises(drs.KernelBuildError, match="--source is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))


def test_bare_c4_source_keeps_the_tuned_row():
    """--source names the problem: a bare C4 command line still takes the tuner's step-1 row, and the named registers of the source
    term are RY * VX words per set, prefetch depth + 1 sets; with --time-order 2 as well, two such families."""
    args = ["--3d", "--dtype", "fp32"]
    rc0, msg0, src0 = drs.generate(args + [C4])
    rc1, msg1, src1 = drs.generate(args + SOURCE + [C4])
    rc2, msg2, src2 = drs.generate(args + ORDER2 + SOURCE + [C4])
    assert rc0 == rc1 == rc2 == 0
    row = re.search(r"is used \((.*?)\)", msg0).group(1)
    assert "is used (%s)" % row in msg1 and "is used (%s)" % row in msg2
    assert "sv1_0_0" in src1 and "sv2_0_0" not in src1 and "ov0_" not in src1
    assert "sv1_0_0" in src2 and "ov1_0_0" in src2
    i0, i1, i2 = (_info(s) for s in (src0, src1, src2))
    sets = 2
    assert i1["reg_demand"] == i0["reg_demand"] + i0["points_per_lane"] * sets and "source" not in i0
    assert i2["reg_demand"] == i0["reg_demand"] + 2 * i0["points_per_lane"] * sets


def test_no_trace_without_source():
    """A command line without --source emits no trace of the third array."""
    seen = 0
    for cid, ndim, stc, opts in GPU_SMALL[::7] + [("c4", 3, C4, ["--3d", "--dtype", "fp32", "--step", "2"]), ("c4o2", 3, C4, ["--3d", "--dtype", "fp32"] + ORDER2)]:
        rc, msg, src = drs.generate(opts + [stc])
        assert src is None or ("psrc" not in src and "sv0_" not in src and "d_src" not in src and '"source' not in src and "_src(" not in src), cid
        seen += src is not None
    assert seen >= 6


# ---- emulated kernels against the host reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,src,opts", ALL, ids=[c[0] for c in ALL])
def test_emulated_source_bit_exact(tmp_path, monkeypatch, cid, ndim, src, opts):
    """2 launches (both directions of the ping-pong) and 5 (an odd count) from random A, B and F, in both fiber orders of the emulator;
    the gold kernel against the same reference."""
    stc = _small_stc(tmp_path, src, ndim, _dims(cid))
    lib = build_emulated(tmp_path, stc, opts)
    info = json.loads(lib.drs_plugin_info().decode())
    assert info["source"] == 1 and info["stages"] == 1 and info.get("time_order", 1) == (2 if cid.endswith("_order2") else 1)
    _check_bit_exact(lib, oracle.Spec(stc, ndim, 1), opts, ndim, tmp_path, monkeypatch)


@pytest.mark.parametrize("cid,bopts", [("periodic", PERIODIC), ("channel", CHANNEL)])
def test_emulated_source_with_ring_fill(tmp_path, monkeypatch, cid, bopts):
    """Non-fixed boundaries: the host fill of `in`, the sweep, the addition.  F's ring is never touched (bit-equal F is asserted)."""
    stc = _small_stc(tmp_path, stc_path("t3_wave"), 3, (14, 19, 140))
    opts = ["--3d", "--dtype", "fp32", "--sn", "8", "--prefetch"] + bopts + SOURCE
    lib = build_emulated(tmp_path, stc, opts)
    _check_bit_exact(lib, oracle.Spec(stc, 3, 1), opts, 3, tmp_path, monkeypatch, counts=(2, 3), gold_counts=(3,), reverse_counts=())


XTALK = [c for c in SMALL if c[0] in ("3d_star_fp32", "3d_star_oddN_fp64_elem")]


@pytest.mark.parametrize("cid,ndim,src,opts", XTALK, ids=[c[0] for c in XTALK])
def test_source_value_reaches_only_its_own_cell(tmp_path, cid, ndim, src, opts):
    """NaN in single interior cells of F: the result holds NaN in exactly those cells (a source value loaded from a neighbouring cell,
    row or plane would move or spread them)."""
    stc = _small_stc(tmp_path, src, ndim, DIMS[cid])
    lib = build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, 1)
    H = spec.halo
    L, M, N = spec.shape
    # a first-block corner, a last-block corner, mid-grid and the tile edge at x = 255 / 256
    cells = [(H, H, H), (L - H - 1, M - H - 1, N - H - 1), (L // 2, M // 2, N // 2), (H + 1, M - H - 1, 255), (9, 32, 256)]
    for cell in cells:
        cell = tuple(min(max(c, H), n - H - 1) for c, n in zip(cell, spec.shape))
        A, B, F = _inputs(spec, _dt(opts))
        F[cell] = np.nan
        assert lib.drs_plugin_launch_src(A.ctypes.data, B.ctypes.data, F.ctypes.data, None) == 0
        where = np.argwhere(np.isnan(B))
        assert where.shape[0] == 1 and tuple(where[0]) == cell, (cid, cell, where[:4])


# ---- memory contract --------------------------------------------------------------------------------------------------------------
_W256 = ["--bx", "64", "--by", "4", "--block-merge-x", "4", "--block-merge-y", "2", "--sn", "4"]
FOOTPRINT = [(c, n, s, o, DIMS[c]) for c, n, s, o in SMALL if c in ("3d_star_fp32", "3d_store_mask_buffer", "3d_star_oddN_fp64_elem", "2d_star_tile_fp32")] + [
    ("3d_store_mask_buffer_order2", 3, stc_path("t3_star"), [o for c, n, s, o in BOTH if c == "3d_store_mask_buffer_order2"][0], DIMS["3d_store_mask_buffer"]),
    ("edge3_thin", 3, stc_path("edge3_thin"), ["--3d", "--dtype", "fp32"] + SOURCE, None),
    ("edge3_thin_buffer", 3, stc_path("edge3_thin"), ["--3d", "--dtype", "fp32", "--store-mask", "buffer"] + SOURCE, None),
    ("edge3_tile_plus1", 3, stc_path("edge3_tile_plus1"), ["--3d", "--dtype", "fp32"] + _W256 + SOURCE, None),
    ("edge3_tile_plus1_buffer", 3, stc_path("edge3_tile_plus1"), ["--3d", "--dtype", "fp32", "--store-mask", "buffer"] + _W256 + SOURCE, None),
]


@pytest.mark.parametrize("cid,ndim,src,opts,dims", FOOTPRINT, ids=[c[0] for c in FOOTPRINT])
def test_source_memory_contract(tmp_path, cid, ndim, src, opts, dims):
    """All three arrays flush against PROT_NONE pages (end-flush and start-flush), NaN in every unread cell of `in`, in the whole ring
    of F and in the whole ring of `out`: no NaN in out's interior, F bit-unchanged, out's ring bit-unchanged, no SIGSEGV."""
    stc = _small_stc(tmp_path, src, ndim, dims) if dims else src
    if not dims:      # the kernel name is the spec's: keep the edge spec under its own name in a directory of this test
        stc = shutil.copy(src, str(tmp_path))
    lib = build_emulated(tmp_path, stc, opts)
    job = {"so": lib._name, "stc": stc, "ndim": ndim, "dtype": "float32" if "fp32" in opts else "float64", "placements": ["end", "start"],
           "order2": "--time-order" in opts}
    jpath = str(tmp_path / "job.json")
    with open(jpath, "w") as f:
        json.dump(job, f)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "source_child.py"), jpath], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (p.returncode, p.stdout[-1500:], p.stderr[-1500:])


# ---- what a launch reads of src: the emulator-side read log -------------------------------------------------------------------------
READ_LOG = [(c, n, s, o, DIMS[c]) for c, n, s, o in SMALL if c in ("3d_star_fp32", "3d_star_oddN_fp64_elem", "3d_window_prefetch", "3d_dma_fp64", "2d_star_tile_fp32",
                                                                    "2d_odd_stream_fp64")] + [
    ("3d_star_fp32_order2", 3, stc_path("t3_star"), [o for c, n, s, o in BOTH if c == "3d_star_fp32_order2"][0], DIMS["3d_star_fp32"]),
    ("edge3_thin", 3, stc_path("edge3_thin"), ["--3d", "--dtype", "fp32"] + SOURCE, None),
    ("edge3_tile_plus1", 3, stc_path("edge3_tile_plus1"), ["--3d", "--dtype", "fp32"] + _W256 + SOURCE, None),
]


@pytest.mark.parametrize("cid,ndim,src,opts,dims", READ_LOG, ids=[c[0] for c in READ_LOG])
def test_source_ring_is_not_read(tmp_path, cid, ndim, src, opts, dims):
    """The contract's clause "the ring of src is not read", observed: the plugin is compiled with tests/source_readlog.h, which marks
    every byte of src that the extra streams' loads touch.  One launch reads every interior cell of src, whole, and no byte of its ring
    -- also no byte whose value would never reach a store (a partial vector's other elements, a masked row).  16-byte vector rows with
    partial vectors at both x edges, element-wide rows, prefetched and DMA-staged streams, the one-shot 2D tile, with --time-order 2
    (whose old-value loads go to `out`, outside the watched range).  --store-mask buffer is outside this log's reach."""
    assert "--store-mask" not in opts
    stc = _small_stc(tmp_path, src, ndim, dims) if dims else shutil.copy(src, str(tmp_path))
    lib = build_emulated(tmp_path, stc, opts, read_log=True)
    spec = oracle.Spec(stc, ndim, 1)
    dt = _dt(opts)
    A, B, F = _inputs(spec, dt)
    seen = np.zeros(F.nbytes, np.uint8)
    lib.drs_readlog_watch(F.ctypes.data, F.nbytes, seen.ctypes.data)
    assert lib.drs_plugin_launch_src(A.ctypes.data, B.ctypes.data, F.ctypes.data, None) == 0
    lib.drs_readlog_watch(None, 0, None)
    cells = seen.reshape(F.shape + (F.itemsize,))
    assert np.array_equal(cells.all(-1), cells.any(-1))               # whole elements
    read = cells.any(-1)
    inner = np.zeros(F.shape, bool)
    interior(inner, spec.halo)[...] = True
    assert read[inner].all(), (cid, "interior cells of src not read", np.argwhere(inner & ~read)[:4])
    assert not read[~inner].any(), (cid, "ring cells of src read", int(read[~inner].sum()), np.argwhere(read & ~inner)[:4])


# ---- the manufactured fixed point -----------------------------------------------------------------------------------------------------
def test_emulated_fixed_point_fp64(tmp_path):
    """t3_star fp64, u* a product of cosines, F = u* - S(u*) by numpy shifted slices over spec.points (no oracle): one launch from
    in = u* returns u* on the interior within 1e-12, the project's fp64 bar -- only the roundings of one chain and one add are left."""
    cid, ndim, src, opts = FIXED_POINT
    stc = _small_stc(tmp_path, src, ndim, (19, 37, 264))
    lib = build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, 1)
    u, F = fixed_point(spec)
    assert float(np.max(np.abs(interior(F, spec.halo)))) > 1e-3               # the term matters
    out = np.zeros_like(u)
    assert lib.drs_plugin_launch_src(u.ctypes.data, out.ctypes.data, F.ctypes.data, None) == 0
    err = float(np.max(np.abs(interior(out, spec.halo) - interior(u, spec.halo))))
    print("fixed point: max abs error %.3g" % err)
    assert err <= 1e-12, err


# ---- the samples of the tuner's space -------------------------------------------------------------------------------------------------
SMALL_GRID = {3: (13, 21, 300), 2: (1, 37, 300)}       # tiny ragged grids: more than one stream block, a partial x-edge tile
_JOBS = [(which, n) + j for which in SAMPLES for n, j in enumerate(sample_jobs(which))]


def _sample_stc(tmp_path, ndim, path):
    return _small_stc(tmp_path, path, ndim, SMALL_GRID[ndim])


@pytest.mark.parametrize("which,n,ndim,path,dtype,args,step", _JOBS, ids=["%s_%02d" % (j[0], j[1]) for j in _JOBS])
def test_emulated_source_sampled_fuzz(tmp_path, monkeypatch, which, n, ndim, path, dtype, args, step):
    """The two samples (source_cases.sample_jobs) through the CPU emulator on tiny grids: three launches from random A, B and F, dr in
    both fiber orders and gold, bit for bit."""
    stc = _sample_stc(tmp_path, ndim, path)
    opts = args[:-1]
    assert "--source" in opts and ("--time-order" in opts) == (which == "order2_source") and step == 1
    if (which, n) in EMU_REFUSED:       # known before the test runs, with its exact reason; the same line without --source is refused alike
        for o in (opts, [x for x in opts if x != "--source"]):
            p = _cli(o + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
            assert p.returncode == 255 and p.stdout == "Invalid configuration!\n" and p.stderr.splitlines()[-1] == EMU_REFUSED[(which, n)], (o, p.stdout, p.stderr)
        return
    lib = build_emulated(tmp_path, stc, opts)
    _check_bit_exact(lib, oracle.Spec(stc, ndim, 1), opts, ndim, tmp_path, monkeypatch, counts=(3,), gold_counts=(3,), reverse_counts=(3,))


def test_emulated_source_sample_size(tmp_path):
    """20 configurations per sample; on the tiny grids the generator accepts every member outside source_cases.EMU_REFUSED (asked here
    without compiling) and emits a kernel that takes the third array, and at least three quarters of each sample are accepted.  The
    issue's three-quarters rule counts the runtime's refusals at the named specs' sizes too (kernels that spill): those are known when
    build() cross-compiles (16 of 20 and 18 of 20 built, source_cases' docstring) and asserted over the kernel cache by
    tests/test_source_gpu.py."""
    for which in SAMPLES:
        jobs = sample_jobs(which)
        assert len(jobs) == 20 and jobs == sample_jobs(which)
        ok = 0
        for n, (ndim, path, dtype, args, step) in enumerate(jobs):
            rc, msg, src = drs.generate(args[:-1] + [_sample_stc(tmp_path, ndim, path)])
            if (which, n) in EMU_REFUSED:
                assert rc == 255 and src is None, (which, n, msg)
                continue
            assert rc == 0 and src is not None and "psrc" in src and "drs_plugin_launch_src(" in src, (which, n, rc, msg)
            assert ("ov0_0_0" in src) == (which == "order2_source"), (which, n)
            ok += 1
        assert ok >= MIN_CHECKED and ok + sum(1 for k in EMU_REFUSED if k[0] == which) == 20, (which, ok)
