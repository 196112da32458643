"""Random stencil shapes in every problem mode without a GPU: the 12 committed shapes of tests/shape_mode_cases.py on tiny ragged grids
under the CPU emulation (tests/emu), one random configuration of the tuner's space per shape and mode (fixed, periodic, reflect, a
per-axis triple, order 2, source, order 2 + source, the last with a per-axis triple): three launches from random A, random B and random
F, dr_ in the forward fiber order (order 2 and source: in the reverse one too) and gold_, against the host references of
tests/options_reference.py -- bit for bit for single-pass kernels, within 1e-6 (fp32) / 1e-12 (fp64) on non-negative data for temporal
pipelines.  Also: the sample has the shapes the hand-drawn specs lack, the generator's note on reflecting axes names exactly the axes
along which a drawn shape is not its own mirror image, and the jobs of the older samples did not move.  The GPU side
is tests/test_shape_modes_gpu.py."""
import hashlib
import json
import os
import re
import shutil

import numpy as np
import pytest

import drstencil_amd as drs
import fuzz_parity
import oracle
import shape_mode_cases as sm
from options_reference import compare_options_run, options_reference
from emu_util import DRSTENCIL, build_emulated
from helpers import write_stc
from source_cases import build_emulated as build_emulated_source, load_emulated

LAUNCHES = 3            # an odd count: both directions of the ping-pong, the run ends on B
_JOBS = [(mode,) + j for mode in sm.MODES for j in sm.sample_jobs(mode, emulated=True)]


def test_sample_has_the_shapes_the_hand_drawn_specs_lack():
    shapes = sm.shapes()
    assert len(shapes) == sm.N_SHAPES == 12 and sm.MIN_CHECKED * 4 == 3 * sm.N_SHAPES
    assert {s[1] for s in shapes} == {2, 3} and {s[2] for s in shapes} == {1, 2}
    tr = [sm.traits(sm.shape_points(p, nd)[0], nd) for _, nd, _, p in shapes]
    assert sum(a for a, _ in tr) >= 2 and sum(b for _, b in tr) >= 2              # one-sided along the streamed dimension / no centre
    vec = [oracle.Spec(p, nd, 1).dims[2] % 4 == 0 for _, nd, _, p in shapes]
    assert any(vec) and not all(vec)                                              # rows of 16-byte vectors, and not
    for name, nd, h, p in shapes:
        assert oracle.Spec(p, nd, 1).halo == h and os.path.getsize(p) < 8192
        assert min(oracle.Spec(p, nd, 1).shape) >= 3 * 3 * h or nd == 3           # every 2D axis carries three Halos at step 3
    for mode in sm.MODES:
        jobs = sm.sample_jobs(mode)
        assert jobs == sm.sample_jobs(mode) and len(jobs) == 12 and {j[4] for j in jobs} == {"fp32", "fp64"}
        if mode in sm.STEP1:
            assert all(j[6] == 1 and "--temporal" not in j[5] for j in jobs)
        for sid, ndim, stc, dims, dtype, opts, step in jobs:
            assert all(d >= 3 * oracle.Spec(stc, ndim, step).halo for d in dims[3 - ndim:]), sid       # the grid allows the mode
    assert {j[6] for m in ("fixed", "periodic", "reflect", "mixed") for j in sm.sample_jobs(m)} == {1, 2, 3}


def test_older_samples_did_not_move():
    """mode_fuzz_cases.sample_jobs, boundary_cases.sample_jobs and source_cases.sample_jobs return what they returned before
    fuzz_parity learnt the reflect / mixed / source / order2_source modes (digests recorded from the version without them): same
    argument lists, hence the same kernel cache keys and the same counts printed by __graft_entry__.build()."""
    import boundary_cases
    import mode_fuzz_cases
    import source_cases

    def digest(jobs):
        return hashlib.sha256(json.dumps([[j[0], os.path.basename(j[1]), j[2], j[3][:-1], j[4]] for j in jobs]).encode()).hexdigest()[:16]
    assert {m: digest(mode_fuzz_cases.sample_jobs(m)) for m in mode_fuzz_cases.MODES} == \
        {"periodic": "e2438a32004afb9f", "order2": "2c709ff46c8fe9af", "order2_periodic": "d4aec34bb72d654a"}
    assert digest(boundary_cases.sample_jobs()) == "846072a1ebd4676d"
    assert {w: digest(source_cases.sample_jobs(w)) for w in source_cases.SAMPLES} == {"source": "d09752ddb070bb02", "order2_source": "0bf72119efa2fb74"}


def test_new_modes_of_the_manual_sweeps():
    """fuzz_parity.py / fuzz_shapes.py --mode reflect | mixed | source | order2_source: jobs that name their mode, step 1 without
    on-chip stages where the generator asks for it."""
    assert fuzz_parity.MODES[:4] == ("fixed", "periodic", "order2", "order2_periodic") and set(fuzz_parity.MODES[4:]) == {"reflect", "mixed", "source", "order2_source"}
    for mode in fuzz_parity.MODES[4:]:
        jobs = fuzz_parity.make_jobs(18, 3, mode)
        assert len(jobs) == 18 and all(fuzz_parity.job_mode(j[3]) == mode for j in jobs) and jobs == fuzz_parity.make_jobs(18, 3, mode)
        if mode in fuzz_parity.STEP1_MODES:
            assert all(j[4] == 1 and "--temporal" not in j[3] for j in jobs)


def _stc(tmp_path, src, ndim, dims):
    path = str(tmp_path / os.path.basename(src))
    write_stc(path, ndim, dims, 4, sm.shape_points(src, ndim)[0])
    return path


def _generate(stc, opts):
    """(return code, stdout + stderr) of the generator, nothing written."""
    import subprocess
    p = subprocess.run([DRSTENCIL] + list(opts) + ["-o", os.devnull, os.path.basename(stc)], cwd=os.path.dirname(stc), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


def test_emulated_shape_sample_size(tmp_path):
    """At most one quarter of the sample, and of every mode's 12, rejected by the generator (asked here without compiling anything),
    each with a known message; and for the reflecting modes the generator's note names exactly the reflecting axes along which the
    shape is not its own mirror image (step > 1 only: a one-step launch is the mirrored update whatever the shape)."""
    rejected = {m: [] for m in sm.MODES}
    noted = 0
    for mode, sid, ndim, src, dims, dtype, opts, step in _JOBS:
        stc = _stc(tmp_path, src, ndim, dims)
        rc, out = _generate(stc, opts)
        if rc != 0:
            assert any(k in out for k in sm.KNOWN_REFUSALS), (sid, out[-300:])
            rejected[mode].append(sid)
            continue
        m = re.search(r"note: the one-step stencil is not symmetric along the reflecting axis ([zyx, ]+):", out)
        odd = sm.asymmetric_reflecting_axes(sm.shape_points(src, ndim)[0], ndim, opts) if step > 1 else []
        assert (m.group(1).split(", ") if m else []) == odd, (sid, out[-600:])
        noted += bool(odd)
    assert all(len(r) * 4 <= sm.N_SHAPES for r in rejected.values()), rejected
    assert noted >= 2, noted              # the rule was tested on some shape


def _second(lib, tmp_path, source):
    """The same plugin loaded a second time (a copy of the file): the emulator reads EMU_ORDER once per loaded object."""
    import ctypes
    cp = os.path.join(str(tmp_path), "rev_" + os.path.basename(lib._name))
    shutil.copy(lib._name, cp)
    if source:
        return load_emulated(cp)
    rev = ctypes.CDLL(cp)
    rev.drs_plugin_launch.argtypes = [ctypes.c_void_p] * 3
    return rev


@pytest.mark.parametrize("mode,sid,ndim,src,dims,dtype,opts,step", _JOBS, ids=[j[1] for j in _JOBS])
def test_emulated_shape_modes(tmp_path, monkeypatch, mode, sid, ndim, src, dims, dtype, opts, step):
    stc = _stc(tmp_path, src, ndim, dims)
    source = "--source" in opts
    try:
        lib = (build_emulated_source if source else build_emulated)(tmp_path, stc, opts)
    except AssertionError as e:
        assert any(k in str(e) for k in sm.KNOWN_REFUSALS), str(e)[-300:]
        return              # counted by test_emulated_shape_sample_size
    info = json.loads(lib.drs_plugin_info().decode())
    temporal = info.get("stages", 1) > 1
    assert not (temporal and mode in sm.STEP1)
    spec = oracle.Spec(stc, ndim, step)
    A0, B0 = fuzz_parity.mode_inputs(spec, dtype, temporal)
    F0 = fuzz_parity.signed_random(spec.shape, A0.dtype, 13) if source else None
    Ar, Br = A0.copy(), B0.copy()
    assert options_reference(spec, ndim, opts, Ar, Br, F0, LAUNCHES) == LAUNCHES
    assert not np.array_equal(spec.interior(Br), spec.interior(B0)) and not np.array_equal(spec.interior(Ar), spec.interior(A0))

    def run(what, lib_, name, tmp):
        A, B = A0.copy(), B0.copy()
        F = F0.copy() if source else None
        fn = getattr(lib_, name + ("_src" if source else ""))
        for i in range(LAUNCHES):
            s, d = (A, B) if i % 2 == 0 else (B, A)
            assert (fn(s.ctypes.data, d.ctypes.data, F.ctypes.data, None) if source else fn(s.ctypes.data, d.ctypes.data, None)) == 0
        ok, rel = compare_options_run(spec, ndim, opts, dtype, A0, B0, A, B, Ar, Br, LAUNCHES, tmp)
        assert ok and (not source or np.array_equal(F, F0)), (sid, what, rel, int((A != Ar).sum()), int((B != Br).sum()))

    # the emulator latches EMU_ORDER at a loaded object's first launch: the forward runs come first, then a second copy of the plugin
    monkeypatch.delenv("EMU_ORDER", raising=False)
    run("forward", lib, "drs_plugin_launch", temporal)
    run("gold", lib, "drs_plugin_launch_gold", False)
    if mode in sm.STEP1:
        monkeypatch.setenv("EMU_ORDER", "reverse")
        run("reverse", _second(lib, tmp_path, source), "drs_plugin_launch", False)
