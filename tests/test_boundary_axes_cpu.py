"""--boundary reflect and --boundary-x / -y / -z without a GPU: the option surface and its canonical form, the generalised ring-fill
kernel under the CPU emulation (tests/emu) against boundary_cases.host_fill for every combination of modes, whole runs of emitted
kernels against the CPU oracle with that fill in front of every launch, an oracle-free numpy reference, the memory contract flush
against inaccessible pages, the refusals of the slab forms, and a fixed sample of the tuner's space.  The GPU side is
tests/test_boundary_axes_gpu.py."""
import ctypes
import itertools
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import boundary_cases as bc
import drstencil_amd as drs
import fuzz_parity
import oracle
from boundary_cases import MIXED2, MIXED3, MODES, REFLECT, WALLS_X_FIXED, fill_destinations, host_fill, oracle_boundary_run
from emu_util import DRSTENCIL, build_emulated
from helpers import write_stc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = os.path.join(ROOT, "benchmarks", "configs", "c4_3d7pt_star_1024.stc")
LAUNCHES = 3            # an odd count: both directions of the ping-pong, the run ends on B

# one-step stencils with short decimal coefficients.  STAR3 / STAR2 have no symmetry; SYM3 is symmetric along every axis; ZODD3 is
# symmetric along x and y and asymmetric along z
STAR3 = [(0, 0, 0, 0.25), (1, 0, 0, 0.1), (-1, 0, 0, 0.15), (0, 1, 0, 0.12), (0, -1, 0, 0.13), (0, 0, 1, 0.11), (0, 0, -1, 0.14)]
SYM3 = [(0, 0, 0, 0.25), (1, 0, 0, 0.1), (-1, 0, 0, 0.1), (0, 1, 0, 0.12), (0, -1, 0, 0.12), (0, 0, 1, 0.14), (0, 0, -1, 0.14)]
ZODD3 = [(0, 0, 0, 0.25), (1, 0, 0, 0.1), (-1, 0, 0, 0.15), (0, 1, 0, 0.12), (0, -1, 0, 0.12), (0, 0, 1, 0.14), (0, 0, -1, 0.14)]
STAR2 = [(0, 0, 0.3), (1, 0, 0.1), (-1, 0, 0.2), (0, 1, 0.15), (0, -1, 0.25)]
SHAPES = {"STAR3": (3, STAR3), "SYM3": (3, SYM3), "ZODD3": (3, ZODD3), "STAR2": (2, STAR2)}


def _stc(tmp_path, shape, dims, iters=4, name="p"):
    ndim, pts = SHAPES[shape]
    path = os.path.join(str(tmp_path), "%s.stc" % name)
    write_stc(path, ndim, dims, iters, pts)
    return path


def _cli(args, cwd):
    return subprocess.run([DRSTENCIL] + list(args), cwd=cwd, capture_output=True, text=True, timeout=60)


def _info(src):
    return json.loads(re.search(r'drs_plugin_info\(void\)\n\{\n    return "(.*)";', src).group(1).replace('\\"', '"'))


# ---- generator / CLI ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim,dtype", [(3, "fp32"), (3, "fp64"), (2, "fp32"), (2, "fp64")])
@pytest.mark.parametrize("form", ["reflect", "mixed"])
def test_cli_accepts_reflect_and_per_axis(tmp_path, ndim, dtype, form):
    stc = _stc(tmp_path, "STAR3" if ndim == 3 else "STAR2", (10, 12, 16) if ndim == 3 else (1, 12, 16))
    out = str(tmp_path / "k.hip")
    b = REFLECT if form == "reflect" else (MIXED3 if ndim == 3 else MIXED2)
    p = _cli((["--3d"] if ndim == 3 else []) + ["--dtype", dtype, "--step", "2"] + b + ["-o", out, stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "reflect" not in p.stdout and "boundar" not in p.stdout          # stdout stays the reference's protocol
    modes = bc.modes_of(b + [stc], ndim)
    named = ", ".join("%s %s" % (a, m) for a, m in zip("zyx"[3 - ndim:], modes))
    assert "drstencil: note: boundaries per axis: %s; the ring of width 2" % named in p.stderr, p.stderr
    src = open(out).read()
    assert "__global__ void __launch_bounds__(256) wrap_p (real_t* __restrict__ a)" in src
    for ep in ("drs_plugin_launch", "drs_plugin_launch_gold"):
        body = src[src.index('extern "C" int %s(' % ep):]
        assert body.split("\n")[2].strip().startswith("if (int rc = drs_plugin_wrap((void*)in, stream)) return rc;"), ep
    info = _info(src)
    assert info["boundary"] == ("reflect" if form == "reflect" else "mixed") and tuple(info["boundaries"]) == modes and "period" not in info
    assert "// options: " + " ".join((["--3d"] if ndim == 3 else []) + ["--dtype", dtype, "--step", "2"] + b) in src


def test_cli_rejects_bad_values(tmp_path):
    stc = _stc(tmp_path, "STAR3", (10, 12, 16))
    for opt in ("--boundary", "--boundary-x", "--boundary-y", "--boundary-z"):
        for v in ("torus", "Reflect", "mirror", ""):
            p = _cli(["--3d", opt, v, "-o", str(tmp_path / "k.hip"), stc], tmp_path)
            assert p.returncode == 255 and p.stdout == "Illegal input.\n", (opt, v, p.stdout)
        p = _cli(["--3d", opt, stc], tmp_path)                                # a value-taking option in the second-to-last slot
        assert p.returncode == 255 and p.stdout == "Illegal input.\n"
    assert not os.path.exists(str(tmp_path / "k.hip"))


def test_cli_boundary_z_in_2d(tmp_path):
    stc = _stc(tmp_path, "STAR2", (1, 12, 16))
    for v in ("periodic", "reflect"):
        p = _cli(["--dtype", "fp32", "--boundary-z", v, "-o", str(tmp_path / "k.hip"), stc], tmp_path)
        assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", p.stdout
        assert "--boundary-z %s" % v in p.stderr and "2D" in p.stderr, p.stderr
    assert not os.path.exists(str(tmp_path / "k.hip"))
    p = _cli(["--dtype", "fp32", "--boundary-z", "fixed", "-o", str(tmp_path / "k.hip"), stc], tmp_path)
    assert p.returncode == 0 and "wrap_" not in open(str(tmp_path / "k.hip")).read()


def test_cli_three_halo_rule_is_per_axis(tmp_path):
    """10 x 12 x 5 at --step 2 (Halo 2): x is shorter than 3 Halo, so it can only be fixed."""
    stc = _stc(tmp_path, "STAR3", (10, 12, 5))
    base = ["--3d", "--dtype", "fp32", "--step", "2"]
    p = _cli(base + ["--boundary", "periodic", "--boundary-x", "fixed", "-o", str(tmp_path / "k.hip"), stc], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    for b in (["--boundary", "periodic", "--boundary-x", "reflect"], ["--boundary-x", "reflect"], ["--boundary", "reflect"], ["--boundary-x", "periodic"]):
        p = _cli(base + b + ["-o", str(tmp_path / "k2.hip"), stc], tmp_path)
        assert p.returncode == 255 and p.stdout == "Invalid configuration!\n", (b, p.stdout)
        assert "3 * Halo" in p.stderr and "axis x" in p.stderr, p.stderr
    assert not os.path.exists(str(tmp_path / "k2.hip"))
    for dims, axis in (((5, 12, 16), "z"), ((10, 5, 16), "y")):
        stc = _stc(tmp_path, "STAR3", dims, name="q")
        p = _cli(base + ["--boundary-%s" % axis, "reflect", "-o", str(tmp_path / "k2.hip"), stc], tmp_path)
        assert p.returncode == 255 and "axis %s" % axis in p.stderr, p.stderr
        others = [o for a in "zyx" if a != axis for o in ("--boundary-%s" % a, "reflect")]
        assert _cli(base + others + ["-o", str(tmp_path / "k.hip"), stc], tmp_path).returncode == 0


SLAB_BOUNDARIES = [(REFLECT, "--boundary reflect"), (["--boundary-y", "periodic"], "--boundary-y periodic")]


@pytest.mark.parametrize("extra,what", [(["--gpus", "2"], "--gpus N > 1"), (["--pair-launch", "1"], "--pair-launch 1")])
@pytest.mark.parametrize("b,named", SLAB_BOUNDARIES, ids=["reflect", "y_periodic"])
def test_cli_refuses_slab_forms(tmp_path, extra, what, b, named):
    stc = _stc(tmp_path, "STAR3", (16, 12, 16))
    p = _cli(["--3d", "--dtype", "fp32"] + b + extra + ["-o", str(tmp_path / "k.hip"), stc], tmp_path)
    assert p.returncode == 255 and p.stdout == "Invalid configuration!\n"
    assert named + " cannot be combined with " + what in p.stderr, p.stderr
    assert not os.path.exists(str(tmp_path / "k.hip"))


@pytest.mark.parametrize("b,named", SLAB_BOUNDARIES, ids=["reflect", "y_periodic"])
def test_slab_runtimes_refuse(tmp_path, b, named):
    from drstencil_amd import multigpu
    stc = _stc(tmp_path, "STAR3", (16, 12, 16))
    opts = ["--3d", "--dtype", "fp32"] + b
    with pytest.raises(ValueError, match=named):
        multigpu.HipSweep(stc, opts, str(tmp_path))
    with pytest.raises(ValueError, match=named):
        multigpu.HipSweep(stc, ["--3d", "--dtype", "fp32"], str(tmp_path), alone_opts=opts)

    class _Sweep:
        pass
    sw = _Sweep()
    sw.opts = opts
    with pytest.raises(ValueError, match=named):
        multigpu.SlabRun(None, None, (16, 12, 16), 1, 1, 4, 0, 2, sw, None, None)
    with pytest.raises(ValueError, match=named):
        multigpu.NativeSlabRun(None, None, stc, opts, (16, 12, 16), 1, 1, 4, 0, 2, None, None)
    with pytest.raises(drs.KernelBuildError, match=named + " is not supported by the slab runtime"):
        drs.Slab(opts + [stc], world=2, rank=0, cache_dir=str(tmp_path))
    assert not [f for f in os.listdir(str(tmp_path)) if not f.endswith(".stc")]        # no file was written
    # fixed spelled per axis is no refusal, and the periodic message stands as it was
    multigpu.refuse_periodic(["--3d", "--boundary-x", "fixed", "--boundary", "fixed"], "t")
    with pytest.raises(ValueError, match="--boundary periodic is not supported"):
        multigpu.refuse_periodic(["--boundary-x", "periodic", "--boundary-y", "periodic", "--boundary-z", "periodic"], "t")


def test_asymmetric_stencil_note(tmp_path):
    note = "is not symmetric along the reflecting axis"
    asym = _stc(tmp_path, "STAR3", (12, 12, 16), name="a")
    sym = _stc(tmp_path, "SYM3", (12, 12, 16), name="s")
    zodd = _stc(tmp_path, "ZODD3", (12, 12, 16), name="z")
    base = ["--3d", "--dtype", "fp64"]

    def notes(stc, extra):
        rc, msg, src = drs.generate(base + extra + [stc])
        assert rc == 0, msg
        return [ln for ln in msg.splitlines() if note in ln]
    got = notes(asym, ["--step", "2"] + REFLECT)
    assert len(got) == 1 and got[0].startswith("drstencil: note: ") and "axis z, y, x" in got[0], got
    assert notes(asym, REFLECT) == []                                         # one step per launch: nothing is fused
    assert notes(sym, ["--step", "2"] + REFLECT) == []
    assert notes(asym, ["--step", "2", "--boundary", "periodic"]) == []
    got = notes(zodd, ["--step", "2"] + REFLECT)
    assert len(got) == 1 and "axis z:" in got[0], got
    assert notes(zodd, ["--step", "2"] + REFLECT + ["--boundary-z", "periodic"]) == []
    p = _cli(base + ["--step", "2"] + REFLECT + ["-o", str(tmp_path / "k.hip"), asym], tmp_path)
    assert p.returncode == 0 and note in p.stderr and note not in p.stdout


def test_canonical_forms(tmp_path):
    """Three equal per-axis values are --boundary v; all-fixed leaves no trace; the banner and the source carry the canonical form."""
    stc3 = _stc(tmp_path, "STAR3", (10, 12, 16), name="c3")
    stc2 = _stc(tmp_path, "STAR2", (1, 12, 16), name="c2")
    for stc, pre, axes in ((stc3, ["--3d", "--dtype", "fp32", "--step", "2"], "zyx"), (stc2, ["--dtype", "fp64"], "yx")):
        fixed = drs.generate(pre + [stc])
        for v in ("periodic", "reflect"):
            want = drs.generate(pre + ["--boundary", v, stc])
            assert want[0] == 0 and "wrap_" in want[2]
            per_axis = [o for a in axes for o in ("--boundary-%s" % a, v)]
            assert drs.generate(pre + per_axis + [stc]) == want
            assert drs.generate(pre + [o for a in reversed(axes) for o in ("--boundary-%s" % a, v)] + [stc]) == want
            assert drs.generate(pre + ["--boundary", "fixed"] + per_axis + [stc]) == want
            assert drs.generate(pre + ["--boundary", v, "--boundary-x", v, stc]) == want
        for spelled in (["--boundary", "fixed"], [o for a in axes for o in ("--boundary-%s" % a, "fixed")], ["--boundary", "reflect"] + [o for a in axes for o in ("--boundary-%s" % a, "fixed")]):
            assert drs.generate(pre + spelled + [stc]) == fixed, spelled
        # a mixed command: every axis spelled in z, y, x order, whatever the order on the line
        a = drs.generate(pre + ["--boundary", "reflect", "--boundary-x", "fixed", stc])
        b = drs.generate(pre + ["--boundary-x", "fixed"] + [o for ax in axes[:-1] for o in ("--boundary-%s" % ax, "reflect")] + [stc])
        assert a == b and a[0] == 0
        assert "// options: " + " ".join(pre + [o for ax in axes[:-1] for o in ("--boundary-%s" % ax, "reflect")] + ["--boundary-x", "fixed"]) + "\n" in a[2]
    # 2D: --boundary-z fixed beside two equal values is still --boundary v
    assert drs.generate(["--dtype", "fp64", "--boundary-z", "fixed", "--boundary-y", "reflect", "--boundary-x", "reflect", stc2]) == drs.generate(["--dtype", "fp64"] + REFLECT + [stc2])


def test_bare_c4_reflect_keeps_the_tuned_row():
    args = ["--3d", "--dtype", "fp32", "--step", "2"]
    rc0, msg0, src0 = drs.generate(args + [C4])
    for b in (REFLECT, ["--boundary-x", "reflect"], MIXED3):
        rc1, msg1, src1 = drs.generate(args + b + [C4])
        assert rc0 == rc1 == 0
        row = re.search(r"is used \((.*?)\)", msg0).group(1)
        assert "is used (%s)" % row in msg1, msg1

        def sweep_part(src):
            return src[src.index("#include"):src.index("// naive reference kernel")]
        assert sweep_part(src0) == sweep_part(src1)
        assert "wrap_c4_3d7pt_star_1024" in src1 and "wrap_" not in src0


# ---- the fill kernel under the emulation ----------------------------------------------------------------------------------------------
def _emulated(tmp_path, stc, opts):
    lib = build_emulated(tmp_path, stc, opts)
    lib.drs_plugin_wrap.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _axis_opts(modes):
    return [o for a, m in zip(("--boundary-z", "--boundary-y", "--boundary-x")[3 - len(modes):], modes) for o in (a, m)]


FILL_GRIDS = [
    # (id, shape, dims, options, H): the element path, the vector path (fp64 at H = 2: a left ghost vector holds two reversed elements), 2D
    ("7x9x13_fp32_elem", "STAR3", (7, 9, 13), ["--3d", "--dtype", "fp32", "--step", "2"], 2),
    ("6x10x16_fp64_vec", "STAR3", (6, 10, 16), ["--3d", "--dtype", "fp64", "--step", "2"], 2),
    ("12x12_fp32_h4", "STAR2", (1, 12, 12), ["--dtype", "fp32", "--step", "4"], 4),
]
FILL_CASES = [(g, m) for g in FILL_GRIDS for m in itertools.product(MODES, repeat=3 if "--3d" in g[3] else 2)]


@pytest.mark.parametrize("grid,modes", FILL_CASES, ids=["%s_%s" % (g[0], "_".join(m)) for g, m in FILL_CASES])
def test_emulated_fill_equals_host_fill(tmp_path, grid, modes):
    cid, shape, dims, opts, H = grid
    stc = _stc(tmp_path, shape, dims)
    rc, msg, src = drs.generate(opts + _axis_opts(modes) + [stc])
    assert rc == 0, msg
    if all(m == "fixed" for m in modes):
        assert "wrap_" not in src
        return
    lib = _emulated(tmp_path, stc, opts + _axis_opts(modes))
    info = json.loads(lib.drs_plugin_info().decode())
    assert info["halo"] == H
    vec = (dims[2] * (4 if "fp32" in opts else 8)) % 16 == 0
    assert ("drs_wvec_t" in src) == vec, cid
    nd = len(modes)
    a0 = np.random.default_rng(7).random(dims[3 - nd:]).astype(np.float32 if "fp32" in opts else np.float64)      # distinct values everywhere
    assert len(np.unique(a0)) == a0.size
    a = a0.copy()
    assert lib.drs_plugin_wrap(a.ctypes.data, None) == 0
    ref = host_fill(a0.copy(), H, modes)
    assert np.array_equal(a, ref), (cid, modes, np.argwhere(a != ref)[:4])
    dest = fill_destinations(a0.shape, H, modes)
    assert np.array_equal(a[~dest], a0[~dest])                    # the interior and the rings of fixed axes: bit-unchanged
    assert not np.any(a[dest] == a0[dest])                        # every destination was written (all values are distinct)
    inner = a0[tuple(slice(H, n - H) for n in a0.shape)]
    if all(m == "reflect" for m in modes):
        assert np.array_equal(a, np.pad(inner, H, mode="symmetric"))
    if all(m == "periodic" for m in modes):
        assert np.array_equal(a, np.pad(inner, H, mode="wrap"))


# ---- whole runs under the emulation ---------------------------------------------------------------------------------------------------
def _points(src, ndim):
    return [tuple(off[3 - ndim:]) + (c,) for off, c in oracle.Spec(src, ndim, 1).points]


def _tiny_dims(ndim, src):
    """Small ragged grids for the emulator (one fiber per lane): rows of a multiple of 16 bytes, odd ones for the odd-N specs."""
    odd = "odd" in os.path.basename(src)
    if ndim == 3:
        return (13, 17, 135) if odd else (14, 19, 136)
    return (1, 37, 135) if odd else (1, 41, 136)


def _second_lib(lib, tmp_path, tag):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    cp = os.path.join(str(tmp_path), tag + "_" + os.path.basename(lib._name))
    shutil.copy(lib._name, cp)
    rev = ctypes.CDLL(cp)
    rev.drs_plugin_launch.argtypes = [ctypes.c_void_p] * 3
    return rev


def _launches(fn, A, B, n):
    for i in range(n):
        s, d = (A, B) if i % 2 == 0 else (B, A)
        assert fn(s.ctypes.data, d.ctypes.data, None) == 0


def _check_run(lib, stc, ndim, step, opts, tmp_path, monkeypatch, launches=LAUNCHES):
    """dr in both fiber orders and gold, `launches` launches from random A and B, against the oracle with host_fill in front of every
    launch: bit for bit for single-pass kernels, within 1e-6 / 1e-12 for on-chip pipelines (non-negative data); the array filled last
    is its own host fill; cells that no fill and no sweep may write are bit-unchanged."""
    info = json.loads(lib.drs_plugin_info().decode())
    modes = bc.modes_of(opts + [stc], ndim)
    assert tuple(info.get("boundaries", ())) == modes, info
    temporal = info.get("stages", 1) > 1
    order2 = info.get("time_order", 1) == 2
    dtype = "fp32" if "fp32" in opts else "fp64"
    spec = oracle.Spec(stc, ndim, step)
    H = spec.halo
    A0, B0 = fuzz_parity.mode_inputs(spec, dtype, temporal)
    Ar, Br = A0.copy(), B0.copy()
    assert oracle_boundary_run(spec, Ar, Br, modes, launches, order2=order2) == launches
    assert not np.array_equal(spec.interior(Br), spec.interior(B0))
    dest = fill_destinations(A0.shape, H, modes)
    frozen = fuzz_parity.ring_mask(A0.shape, H) & ~dest
    last = "A" if launches % 2 else "B"                  # launch n - 1 fills its input: A for an odd count

    def run(what, fn, tmp):
        A, B = A0.copy(), B0.copy()
        _launches(fn, A, B, launches)
        assert np.array_equal(A[frozen], A0[frozen]) and np.array_equal(B[frozen], B0[frozen]), what
        filled = A if last == "A" else B
        assert np.array_equal(filled, host_fill(filled.copy(), H, modes)), what
        if tmp:
            rel = max(fuzz_parity.rel_error(A, Ar), fuzz_parity.rel_error(B, Br))
            assert rel <= (1e-6 if dtype == "fp32" else 1e-12), (what, rel)
        else:
            assert np.array_equal(A, Ar) and np.array_equal(B, Br), (what, int((A != Ar).sum()), int((B != Br).sum()))

    monkeypatch.delenv("EMU_ORDER", raising=False)
    run("forward", lib.drs_plugin_launch, temporal)
    run("gold", lib.drs_plugin_launch_gold, False)
    monkeypatch.setenv("EMU_ORDER", "reverse")
    run("reverse", _second_lib(lib, tmp_path, "rev").drs_plugin_launch, temporal)
    return info


RUN_CASES = bc.small_cases() + bc.wave_cases_reflect()


@pytest.mark.parametrize("cid,ndim,src,opts", RUN_CASES, ids=[c[0] for c in RUN_CASES])
def test_emulated_run_vs_oracle_with_fill(tmp_path, monkeypatch, cid, ndim, src, opts):
    step = int(opts[opts.index("--step") + 1]) if "--step" in opts else 1
    stc = str(tmp_path / "r.stc")
    write_stc(stc, ndim, _tiny_dims(ndim, src), 4, _points(src, ndim))
    lib = build_emulated(tmp_path, stc, opts)
    info = _check_run(lib, stc, ndim, step, opts, tmp_path, monkeypatch)
    assert (info.get("stages", 1) > 1) == ("--temporal" in opts), info


# ---- semantics without the oracle -------------------------------------------------------------------------------------------------------
def test_emulated_fused_step2_equals_padded_numpy_steps(tmp_path):
    """Walls in x and y (the stencil is symmetric along both), periodic and asymmetric in z: fused step-2 launches (fp64) == that many
    one-step updates in float64 numpy, each on the array padded by `symmetric` / `wrap` per axis."""
    dims = (10, 12, 14)
    stc = _stc(tmp_path, "ZODD3", dims, iters=4)
    lib = _emulated(tmp_path, stc, ["--3d", "--dtype", "fp64", "--step", "2"] + REFLECT + ["--boundary-z", "periodic"])
    H = 2
    A0 = np.random.default_rng(5).random(dims)
    A, B = A0.copy(), np.zeros_like(A0)
    _launches(lib.drs_plugin_launch, A, B, 2)

    def steps(u, n):
        for _ in range(n):
            p = np.pad(u, ((1, 1), (0, 0), (0, 0)), mode="wrap")
            p = np.pad(p, ((0, 0), (1, 1), (1, 1)), mode="symmetric")
            v = np.zeros_like(u)
            for k, j, i, c in ZODD3:
                v += c * p[1 + k:1 + k + u.shape[0], 1 + j:1 + j + u.shape[1], 1 + i:1 + i + u.shape[2]]
            u = v
        return u
    inner = tuple(slice(H, n - H) for n in dims)
    ref1 = steps(A0[inner], 2)
    ref2 = steps(ref1, 2)
    for got, ref in ((B[inner], ref1), (A[inner], ref2)):
        rel = np.max(np.abs(got - ref) / np.abs(ref))
        assert rel <= 1e-12, rel


# ---- memory contract ----------------------------------------------------------------------------------------------------------------------
CONTRACT = [c for c in bc.edge_cases() if c[0] in ("min_333_fp32_reflect_modest", "min_333_fp32_reflect_default", "thin_7x9x13_fp32_s2_mixed_modest",
                                                    "thin_7x9x13_fp64_s2_mixed_default")]
CONTRACT += [("thin_7x9x13_fp32_s2_reflect_modest", 3, bc.stc("edge3_thin"), ["--3d", "--dtype", "fp32", "--step", "2"] + REFLECT + ["--bx", "16", "--by", "4", "--block-merge-y", "2", "--sn", "4"]),
             ("thin_7x9x13_fp64_s2_reflect_xfixed", 3, bc.stc("edge3_thin"), ["--3d", "--dtype", "fp64", "--step", "2"] + WALLS_X_FIXED)]


@pytest.mark.parametrize("cid,ndim,stc,opts", CONTRACT, ids=[c[0] for c in CONTRACT])
def test_memory_contract_flush_against_guard_pages(tmp_path, cid, ndim, stc, opts):
    """Both arrays flush against PROT_NONE pages (end-flush and start-flush), NaN in every cell that is neither read nor a fill source:
    no SIGSEGV, no NaN in the output's interior, the output's ring untouched, and the input outside the fill's destinations -- the
    rings of fixed axes included -- bit-unchanged (tests/boundary_child.py)."""
    lib = build_emulated(tmp_path, stc, opts)
    step = int(opts[opts.index("--step") + 1]) if "--step" in opts else 1
    job = {"so": lib._name, "stc": stc, "ndim": ndim, "step": step, "dtype": "float32" if "fp32" in opts else "float64",
           "modes": list(bc.modes_of(opts + [stc], ndim)), "placements": ["end", "start"]}
    jpath = str(tmp_path / "job.json")
    with open(jpath, "w") as f:
        json.dump(job, f)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "boundary_child.py"), jpath], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("DONE"), (p.returncode, p.stdout[-1500:], p.stderr[-1500:])


# ---- a fixed sample of the tuner's space ----------------------------------------------------------------------------------------------
def _fuzz_dims(job):
    ndim, path = job[0], job[1]
    order = oracle.Spec(path, ndim, 1).halo
    return (13, 21, 300) if ndim == 3 else ((37, 300) if order == 1 else (29, 280))


def _fuzz_jobs():
    return bc.sample_jobs(shape_of=_fuzz_dims)


def test_emulated_boundary_sampled_fuzz(tmp_path, monkeypatch):
    """The 20 configurations of boundary_cases.sample_jobs on tiny grids, each with its per-axis triple (axes the tiny grid cannot carry
    stay fixed): three launches, both fiber orders and gold.  At least 15 are checked; the others are rejections by the generator."""
    jobs = _fuzz_jobs()
    assert len(jobs) == bc.SAMPLE[0] == 20
    checked, rejected = 0, []
    for n, (ndim, path, dtype, args, step) in enumerate(jobs):
        work = tmp_path / ("j%02d" % n)
        work.mkdir()
        stc = str(work / "f.stc")
        dims = _fuzz_dims(jobs[n])
        write_stc(stc, ndim, dims if ndim == 3 else (1,) + dims, 4, _points(path, ndim))
        opts = args[:-1]
        modes = bc.modes_of(args, ndim)
        assert any(m != "fixed" for m in modes), args
        rc, msg, src = drs.generate(opts + [stc])
        if rc != 0:
            assert "Invalid configuration" in msg, msg
            rejected.append(" ".join(opts))
            continue
        lib = build_emulated(work, stc, opts)
        _check_run(lib, stc, ndim, step, opts, work, monkeypatch)
        checked += 1
    print("boundary fuzz (emulated): %d checked, %d rejected by the generator" % (checked, len(rejected)))
    assert checked >= bc.MIN_CHECKED, (checked, rejected)
