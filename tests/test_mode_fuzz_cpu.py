"""--boundary periodic and --time-order 2 over the tuner's space without a GPU: a fixed-seed sample of random configurations per
problem mode (periodic, order 2, order 2 + periodic) under the CPU emulation (tests/emu), built the way
test_emulated_kernels._emulated_fuzz_jobs builds its own and compared with the host references of tests/fuzz_parity.py; explicit
order-2 cases for the knobs the seeded cases of tests/wave_cases.py do not reach; the edge grids of tests/mode_fuzz_cases.py; and
the guarantee that the fixed-boundary fuzz sample of the GPU suite did not move.  The GPU side is tests/test_mode_fuzz_gpu.py."""
import hashlib
import json
import os
import shutil

import numpy as np
import pytest

import fuzz_parity
import oracle
from emu_util import build_emulated
from helpers import write_stc
from mode_fuzz_cases import EDGE, ROLL_IDS
from periodic_cases import roll_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("periodic", "order2", "order2_periodic")
SAMPLE = (14, 4)        # (configurations per mode, seed): 12 or more per mode once the lane filter has thinned the space
LAUNCHES = 3            # an odd count: both directions of the ping-pong, the run ends on B


def _stc_path(name):
    return os.path.join(ROOT, "tests", "stc", name + ".stc")


def _points(src, ndim):
    return [tuple(off[3 - ndim:]) + (c,) for off, c in oracle.Spec(src, ndim, 1).points]


def test_fixed_mode_sample_did_not_move():
    """make_jobs(n, seed) and make_jobs(n, seed, "fixed") are the sweep as it was before the mode axis: the prebuilt sample of the GPU
    suite (gpu_cases.FUZZ_SAMPLE) keeps its argument lists, hence its kernel cache keys.  The digest was recorded from the version
    without modes."""
    from gpu_cases import FUZZ_SAMPLE
    jobs = fuzz_parity.make_jobs(*FUZZ_SAMPLE)
    assert jobs == fuzz_parity.make_jobs(*FUZZ_SAMPLE, mode="fixed")
    text = json.dumps([[j[0], os.path.basename(j[1]), j[2], j[3][:-1], j[4]] for j in jobs])
    assert len(jobs) == 56 and all(fuzz_parity.job_mode(j[3]) == "fixed" for j in jobs)
    assert hashlib.sha256(text.encode()).hexdigest()[:16] == "8cfda2a2b13397e1"


def test_mode_jobs_name_their_mode():
    """The GPU sample: 20 jobs per mode, each naming its mode, both dtypes, the same jobs on every call."""
    from mode_fuzz_cases import SAMPLE as GPU_SAMPLE, sample_jobs
    for mode in MODES:
        jobs = sample_jobs(mode)
        assert len(jobs) == GPU_SAMPLE[0] == 20
        assert all(fuzz_parity.job_mode(j[3]) == mode for j in jobs)
        assert {j[2] for j in jobs} == {"fp32", "fp64"}
        if mode.startswith("order2"):          # what the generator accepts: step 1, no on-chip stages
            assert all(j[4] == 1 and "--temporal" not in j[3] for j in jobs)
        else:
            assert {j[4] for j in jobs} == {1, 2, 3}
            assert jobs == sample_jobs(mode)


# ---- the emulated sample ----------------------------------------------------------------------------------------------------------
def _mode_fuzz_jobs(mode, n=SAMPLE[0], seed=SAMPLE[1]):
    """A fixed random sample of the tuner's space in `mode` on the tiny ragged grids of test_emulated_kernels._emulated_fuzz_jobs
    (the emulator runs one fiber per lane: workgroups below 256 lanes), prefetch depths 1-4; periodic steps 1-2 (FUZZ_STEPS widens
    them), order 2 at step 1 without on-chip stages."""
    import random
    from drstencil_amd.tuner import tuning as t
    rnd = random.Random("%s/%d" % (mode, seed))
    order2 = mode.startswith("order2")
    jobs = []
    grids = [(3, "t3_star", (13, 21, 300), 1), (2, "t2_star", (1, 37, 300), 1), (2, "t2_box25", (1, 29, 280), 2)]
    for g, (ndim, src, dims, order) in enumerate(grids):
        for d, dtype in enumerate(("fp32", "fp64")):
            t.order, t.ndim, t.elem_bytes = order, ndim, 4 if dtype == "fp32" else 8
            steps_ = (1,) if order2 else tuple(int(x) for x in os.environ.get("FUZZ_STEPS", "1,2").split(","))
            if order > 1:
                steps_ = tuple(x for x in steps_ if x <= 2) or (2,)
            space = [v for v in t.enumerate_space(steps_) if v[2][0] * v[2][1] <= 256 and v[2][0] <= 68 and v[3] <= 16]
            count = n // 6 + (2 * g + d < n % 6)
            for v in rnd.sample(space, min(len(space), count)):
                cl = t.cfgToCommandLine(v).split()
                if "--prefetch-depth" in cl:
                    cl[cl.index("--prefetch-depth") + 1] = str(rnd.choice([1, 2, 3, 4]))
                if "--schedule" not in cl and rnd.random() < 0.6:
                    cl[cl.index("--merge-forward") + 1] = str(rnd.choice([0, 2, 3, 100]))
                if rnd.random() < 0.3:
                    cl += ["--uniform-loads", str(rnd.choice([1, 2]))]
                if rnd.random() < 0.3:
                    cl += ["--store-mask", "buffer"]
                if rnd.random() < 0.2:
                    cl += ["--drain", str(rnd.choice([1, 2]))]
                if rnd.random() < 0.35 and "--temporal" not in cl and "--cyclic-merge-y" not in cl and (ndim == 3 or "--streaming" in cl):
                    cl += ["--stage", "dma"]
                if rnd.random() < 0.3:
                    cl += ["--defer-stores", "1"]
                fuzz_parity.round3_knobs(rnd, cl)
                fuzz_parity.round4_knobs(rnd, cl)
                if "--skew" in cl and ndim == 2 and "--streaming" not in cl:
                    del cl[cl.index("--skew"):cl.index("--skew") + 2]
                opts = (["--3d"] if ndim == 3 else []) + ["--dtype", dtype] + cl + fuzz_parity.MODE_OPTS[mode]
                jobs.append(("%s_%s_%s_%dd%s" % (mode, t.cfgToString(v), dtype, ndim, src[3:]), mode, ndim, src, dims, opts, v[0]))
    return jobs


_JOBS = [j for m in MODES for j in _mode_fuzz_jobs(m)]


def _second_lib(lib, tmp_path, tag):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    import ctypes
    cp = os.path.join(str(tmp_path), tag + "_" + os.path.basename(lib._name))
    shutil.copy(lib._name, cp)
    rev = ctypes.CDLL(cp)
    rev.drs_plugin_launch.argtypes = [ctypes.c_void_p] * 3
    return rev


def _launches(fn, A, B, n):
    for i in range(n):
        s, d = (A, B) if i % 2 == 0 else (B, A)
        assert fn(s.ctypes.data, d.ctypes.data, None) == 0


def _check_emulated(lib, stc, ndim, step, mode, dtype, tmp_path, monkeypatch, counts=(LAUNCHES,), reverse=None):
    """dr (forward fiber order; order 2: reverse too) and gold for each launch count against the mode's host reference."""
    info = json.loads(lib.drs_plugin_info().decode())
    temporal = info.get("stages", 1) > 1
    assert info.get("time_order", 1) == (2 if mode.startswith("order2") else 1)
    assert (info.get("boundary") == "periodic") == mode.endswith("periodic")
    assert not (temporal and mode != "periodic")
    spec = oracle.Spec(stc, ndim, step)
    A0, B0 = fuzz_parity.mode_inputs(spec, dtype, temporal)
    refs = {}
    for n in counts:
        Ar, Br = A0.copy(), B0.copy()
        assert fuzz_parity.mode_reference(spec, Ar, Br, n, mode) == n
        assert not np.array_equal(spec.interior(Br), spec.interior(B0))
        assert n < 2 or not np.array_equal(spec.interior(Ar), spec.interior(A0))       # no launch of the run is the identity
        refs[n] = (Ar, Br)

    def run(what, fn, tmp):
        for n in counts:
            Ar, Br = refs[n]
            A, B = A0.copy(), B0.copy()
            _launches(fn, A, B, n)
            if tmp and n % 2:         # the ring rule of compare_mode_run speaks of a run that ends on A: swap the roles
                ok, rel = fuzz_parity.compare_mode_run(spec, mode, dtype, B0, A0, B, A, Br, Ar, n, True)
            else:
                ok, rel = fuzz_parity.compare_mode_run(spec, mode, dtype, A0, B0, A, B, Ar, Br, n, tmp)
            assert ok, (what, n, rel, int((A != Ar).sum()), int((B != Br).sum()))

    # the emulator latches EMU_ORDER at a loaded object's first launch: the forward runs come first, then a second copy of the plugin
    monkeypatch.delenv("EMU_ORDER", raising=False)
    run("forward", lib.drs_plugin_launch, temporal)
    run("gold", lib.drs_plugin_launch_gold, False)
    if mode.startswith("order2") if reverse is None else reverse:
        monkeypatch.setenv("EMU_ORDER", "reverse")
        run("reverse", _second_lib(lib, tmp_path, "rev").drs_plugin_launch, temporal)
    return spec


@pytest.mark.parametrize("vid,mode,ndim,src,dims,opts,step", _JOBS, ids=[j[0] for j in _JOBS])
def test_emulated_mode_sampled_fuzz(vid, mode, ndim, src, dims, opts, step, tmp_path, monkeypatch):
    """Random tuner-space configurations with --boundary periodic and / or --time-order 2 through the CPU emulator: three launches
    from random A and random B, dr in the forward fiber order (order 2: and in the reverse one) and gold, against the oracle with the
    host wrap in front of every launch and / or the subtraction of the old output -- the emitter's old-value stream and the wrap
    without the GPU compiler in the loop."""
    stc = str(tmp_path / "f.stc")
    write_stc(stc, ndim, dims, 4, _points(_stc_path(src), ndim))
    try:
        lib = build_emulated(tmp_path, stc, opts)
    except AssertionError as e:
        assert "Invalid configuration" in str(e) or "tile" in str(e) or "halo" in str(e), str(e)[-300:]
        pytest.skip("rejected by the generator")
    _check_emulated(lib, stc, ndim, step, mode, "fp32" if "fp32" in opts else "fp64", tmp_path, monkeypatch)


def test_emulated_mode_sample_size(tmp_path):
    """12 or more configurations per mode, 36 or more in all; at most one quarter of the sample rejected by the generator (asked
    here without compiling anything, so the count does not depend on which cases ran in this process)."""
    import drstencil_amd as drs
    per = {m: sum(1 for j in _JOBS if j[1] == m) for m in MODES}
    assert min(per.values()) >= 12 and len(_JOBS) >= 36, per
    rejected = []
    for vid, mode, ndim, src, dims, opts, step in _JOBS:
        stc = str(tmp_path / ("%s_%d.stc" % (src, ndim)))
        write_stc(stc, ndim, dims, 4, _points(_stc_path(src), ndim))
        if drs.generate(opts + [stc])[0] != 0:
            rejected.append(vid)
    assert len(rejected) * 4 <= len(_JOBS), rejected


# ---- explicit order-2 cases for the knobs no seeded case has --------------------------------------------------------------------------
# grids with partial x-edge tiles and more than one stream block (2D streams: several row blocks); (id, ndim, spec, (L, M, N), options)
KNOBS = [
    ("cyclic_merge_x", 3, "t3_star", (13, 19, 264), ["--3d", "--dtype", "fp32", "--sn", "5", "--cyclic-merge-x", "4", "--bx", "32", "--by", "4", "--block-merge-y", "2"]),
    ("cyclic_merge_y", 3, "t3_star", (15, 29, 140), ["--3d", "--dtype", "fp64", "--sn", "5", "--cyclic-merge-y", "3", "--by", "2", "--bx", "32"]),
    ("loader_waves", 3, "t3_star", (17, 21, 300), ["--3d", "--dtype", "fp32", "--sn", "6", "--stage", "dma", "--loader-waves", "2", "--prefetch-depth", "3"]),
    ("exact_x_0", 3, "t3_star", (19, 23, 300), ["--3d", "--dtype", "fp32", "--sn", "7", "--prefetch", "--exact-x", "0", "--bx", "34", "--by", "7", "--block-merge-y", "2"]),
    ("uniform_loads2_buffer_drain1_oddN_fp64", 3, "t3_star", (12, 17, 263), ["--3d", "--dtype", "fp64", "--sn", "3", "--prefetch", "--prefetch-depth", "2", "--uniform-loads", "2", "--store-mask", "buffer", "--drain", "1"]),
    ("rows_unpacked_defer_stores", 3, "t3_star", (19, 23, 262), ["--3d", "--dtype", "fp32", "--sn", "7", "--prefetch", "--order", "rows", "--pack", "0", "--defer-stores", "1"]),
    ("2d_box_stream_dma_periodic", 2, "t2_box25", (1, 61, 268), ["--dtype", "fp32", "--streaming", "--sn", "9", "--stage", "dma", "--boundary", "periodic"]),
    ("2d_tile_cyclic_merge_x", 2, "t2_box25", (1, 61, 268), ["--dtype", "fp64", "--cyclic-merge-x", "4", "--bx", "32", "--by", "4", "--block-merge-y", "2"]),
    # the PD + 1 register sets of the old-value prefetch at the deepest depth, stream blocks shorter than the depth at the top
    ("prefetch_depth4", 3, "t3_star", (13, 19, 264), ["--3d", "--dtype", "fp32", "--sn", "5", "--prefetch", "--prefetch-depth", "4", "--bx", "32", "--by", "4", "--block-merge-y", "2"]),
]


@pytest.mark.parametrize("cid,ndim,src,dims,opts", KNOBS, ids=[c[0] for c in KNOBS])
def test_emulated_order_2_knobs(tmp_path, monkeypatch, cid, ndim, src, dims, opts):
    """2 and 3 launches (both directions of the ping-pong, an odd count) from random A and random B, both fiber orders and gold, bit
    for bit."""
    stc = str(tmp_path / "k.stc")
    write_stc(stc, ndim, dims, 4, _points(_stc_path(src), ndim))
    opts = opts + ["--time-order", "2"]
    lib = build_emulated(tmp_path, stc, opts)
    info = json.loads(lib.drs_plugin_info().decode())
    mode = fuzz_parity.job_mode(opts)
    spec = _check_emulated(lib, stc, ndim, 1, mode, "fp32" if "fp32" in opts else "fp64", tmp_path, monkeypatch, counts=(2, 3))
    assert info["stream_blocks"] > 1 or not info["streams"], info
    assert (spec.shape[-1] - 2 * spec.halo) % info["tile_owned_cols"] != 0


# ---- the edge grids of the GPU suite, emulated ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,ndim,stc,opts,mode", EDGE, ids=[c[0] for c in EDGE])
def test_emulated_mode_edge_grids(tmp_path, monkeypatch, cid, ndim, stc, opts, mode):
    """The cases of test_mode_fuzz_gpu.py::test_mode_edge_grids under the emulation: the spec's own number of launches."""
    step = int(opts[opts.index("--step") + 1]) if "--step" in opts else 1
    lib = build_emulated(tmp_path, stc, opts)
    spec = oracle.Spec(stc, ndim, step)
    dtype = "fp32" if "fp32" in opts else "fp64"
    _check_emulated(lib, stc, ndim, step, mode, dtype, tmp_path, monkeypatch, counts=(spec.launches,))
    if cid in ROLL_IDS:
        A, B = fuzz_parity.mode_inputs(spec, dtype, False)
        ref = roll_reference(oracle.Spec(stc, ndim, 1).points, spec.interior(A).copy(), spec.launches * step)
        _launches(lib.drs_plugin_launch, A, B, spec.launches)
        assert fuzz_parity.rel_error(spec.interior(A), ref) <= 1e-12


# ---- the extended memory contract on the edge grids and the new knobs ---------------------------------------------------------------------
# A bit-for-bit comparison cannot see an old-value load that lost one of its store's guards: the value it fetches belongs to a lane that
# stores nothing.  What it breaks is the contract -- a launch reads the interior of `out` and nothing else of it -- so these cases run
# with both arrays flush against inaccessible pages (tests/wave_child.py): in the last rows of the last plane such a load leaves the array.
CONTRACT_EDGE = [c for c in EDGE if c[4] == "order2"]
CONTRACT_KNOBS = [c for c in KNOBS if c[0] in ("cyclic_merge_x", "exact_x_0", "uniform_loads2_buffer_drain1_oddN_fp64", "2d_tile_cyclic_merge_x")]


def _memory_contract(tmp_path, lib, stc, ndim, opts):
    import subprocess
    import sys
    job = {"so": lib._name, "stc": stc, "ndim": ndim, "dtype": "float32" if "fp32" in opts else "float64", "placements": ["end", "start"]}
    jpath = str(tmp_path / "job.json")
    with open(jpath, "w") as f:
        json.dump(job, f)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wave_child.py"), jpath], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (p.returncode, p.stdout[-1500:], p.stderr[-1500:])


@pytest.mark.parametrize("cid,ndim,stc,opts,mode", CONTRACT_EDGE, ids=[c[0] for c in CONTRACT_EDGE])
def test_order_2_memory_contract_edge_grids(tmp_path, cid, ndim, stc, opts, mode):
    """Both arrays flush against PROT_NONE pages (end-flush and start-flush), NaN in every unread cell of `in` and in the whole ring of
    `out`: no NaN in out's interior, out's ring bit-unchanged, no SIGSEGV -- on the grid narrower than a tile and on the one whose last
    tile owns a single column."""
    _memory_contract(tmp_path, build_emulated(tmp_path, stc, opts), stc, ndim, opts)


@pytest.mark.parametrize("cid,ndim,src,dims,opts", CONTRACT_KNOBS, ids=[c[0] for c in CONTRACT_KNOBS])
def test_order_2_memory_contract_knobs(tmp_path, cid, ndim, src, dims, opts):
    stc = str(tmp_path / "k.stc")
    write_stc(stc, ndim, dims, 4, _points(_stc_path(src), ndim))
    opts = opts + ["--time-order", "2"]
    _memory_contract(tmp_path, build_emulated(tmp_path, stc, opts), stc, ndim, opts)
