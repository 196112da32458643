"""IEEE special values inside the footprint, without a GPU: a sample of the single-pass kernels of tests/test_special_values_gpu.py
(special_values.emulated_cases) on smaller grids under the CPU emulation (tests/emu), on data that holds +-0.0, subnormals, values up to
the largest finite one, +-inf and NaN (special_values.special_fill; the source array too): two launches of dr_ and of gold_ (both
directions of the ping-pong) against the existing host references, NaN in the same cells and every other cell the same BITS
(special_values.same_bits), on both whole arrays.  The reference alone must keep a quarter of its interior finite and hold every
output class (normal, subnormal, +0.0, -0.0, +inf, -inf, NaN); the grids too small for that are named in special_values.CLASS_WAIVERS, class by class.  Kernels
with on-chip stages (info["stages"] > 1) are left out: they are held to a relative bar, which means nothing on this data.

Tried once by hand, not as a test: with the first tap of the taps-order chain emitted as an FMA onto 0.0 instead of a product
(emit_hip.hpp, emit_scatter), all 1015 tests of the CPU suite from before this module still pass -- 0.0 + c * x equals c * x for every x
but c * x = -0.0 -- and test_special_values_emulated fails in 55 of its 106 cases, the ones whose kernel takes the taps order."""
import json

import numpy as np
import pytest

import oracle
import special_values as sv
from emu_util import build_emulated
from source_cases import build_emulated as build_emulated_source

CASES = sv.emulated_cases()


def test_fill_holds_every_class_and_same_bits_tells_them_apart():
    for dt in (np.float32, np.float64):
        fi = np.finfo(dt)
        a = sv.special_fill((20, 30, 40), dt, 5, 3)
        assert sv.classes_present(a) == set(sv.OUTPUT_CLASSES)
        assert (a == fi.max).any() and (np.abs(a) == fi.smallest_subnormal).any() and (a == fi.tiny * dt(1.5)).any()
        assert np.isfinite(a[10:]).all() and np.isnan(a[:10]).sum() == np.isposinf(a[:10]).sum() == np.isneginf(a[:10]).sum() == round(sv.INF_SHARE * a[:10].size)
        blocks = a[10:19, :30, :39].reshape(3, 3, 10, 3, 13, 3).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 27)
        kinds = {frozenset(sv.classes_present(b)) for b in blocks}
        assert {frozenset(["-0.0"]), frozenset(["+0.0"]), frozenset(["subnormal"])} <= kinds       # whole blocks of one class
        assert np.array_equal(a, sv.special_fill((20, 30, 40), dt, 5, 3), equal_nan=True) and sv.same_bits(a, a.copy())
        z = np.zeros(4, dt)
        assert np.array_equal(z, -z) and not sv.same_bits(z, -z) and sv.count_different(z, -z) == 4
        s = np.full(4, fi.smallest_subnormal, dt)
        assert not sv.same_bits(s, z) and not sv.same_bits(s, 2 * s)
        n = np.array([np.nan, 1.0], dt)
        assert sv.same_bits(n, n.copy()) and not sv.same_bits(n, n[::-1].copy()) and sv.count_different(n, n[::-1].copy()) == 2
        assert sv.same_bits(n, np.array([-np.nan, 1.0], dt))                                         # a NaN is a NaN, whatever its bits


def test_sample_covers_every_family():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids))
    for family in ("parity_", "periodic_", "boundary_", "order2_", "source_", "edge_thin_7x9x13", "edge_tile_plus1", "edge_min_", "edge_source_"):
        assert any(i.startswith(family) for i in ids), family
    assert {"fp32", "fp64"} <= {o[o.index("--dtype") + 1] for _, _, _, o in CASES}
    assert set(ids) <= {c[0] for c in sv.gpu_cases()} and len(sv.gpu_cases()) > 200


@pytest.mark.parametrize("cid,ndim,stc,opts", CASES, ids=[c[0] for c in CASES])
def test_special_values_emulated(tmp_path, cid, ndim, stc, opts):
    stc = sv.emulated_stc(tmp_path, stc, ndim)
    source = "--source" in opts
    lib = (build_emulated_source if source else build_emulated)(tmp_path, stc, opts)
    assert json.loads(lib.drs_plugin_info().decode()).get("stages", 1) == 1
    spec = oracle.Spec(stc, ndim, sv.step_of(opts))
    A0, B0, F0 = sv.inputs(cid, spec, opts)
    Ar, Br = sv.reference(spec, ndim, opts, A0.copy(), B0.copy(), F0)
    sv.assert_conditions(cid, spec, Ar, Br)
    for which in ("launch", "launch_gold"):
        A, B = A0.copy(), B0.copy()
        for s, d in ((A, B), (B, A)):
            if source:
                F = F0.copy()
                assert getattr(lib, "drs_plugin_%s_src" % which)(s.ctypes.data, d.ctypes.data, F.ctypes.data, None) == 0
                assert sv.same_bits(F, F0)
            else:
                assert getattr(lib, "drs_plugin_" + which)(s.ctypes.data, d.ctypes.data, None) == 0
        assert sv.same_bits(A, Ar) and sv.same_bits(B, Br), (cid, which, sv.count_different(A, Ar), sv.count_different(B, Br))
