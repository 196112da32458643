"""IEEE special values inside the footprint (tests/test_special_values_cpu.py, tests/test_special_values_gpu.py): a fill that puts
signed zeros, subnormals, values near the largest finite one, infinities and NaN where kernels read them, and a comparison that tells
-0.0 from +0.0 and one subnormal from another.  Every other test of the project draws uniform data and compares with np.array_equal,
for which -0.0 == 0.0.

The value classes:
    normal in [-1, 1)                   +0.0                    -0.0
    +- subnormals (random)              +- the smallest one     +- 1.5 x the smallest normal (its products with a coefficient are subnormal)
    +- magnitudes up to finfo.max (log-uniform over the top 16 binades, the largest finite value itself included)
    +inf, -inf, NaN: INF_SHARE (2 per mille) each of the per-cell half
One half of the grid, cut along the outermost axis, draws the class per cell: every mix of classes inside one footprint.  The other
half draws it per block of `block` cells an edge (>= 2 Halo + 1, so that some outputs have every tap in one block): outputs whose taps
are all -0.0, all +0.0, all subnormal or all huge, which per-cell draws almost never produce -- the sign of a zero result and a
subnormal result are what a chain started from 0.0, a lane masked by multiplying or a flushed subnormal get wrong.  Blocks hold no inf
and no NaN, so a good part of the outputs stays finite.

The two conditions the tests assert on the REFERENCE alone (reference_conditions): at least a quarter of the interior finite, and every
output class present."""
import numpy as np

INF_SHARE = 0.002
OUTPUT_CLASSES = ("normal", "subnormal", "+0.0", "-0.0", "+inf", "-inf", "nan")
# (class, weight): per cell and per block alike; inf and NaN are placed afterwards, in the per-cell half only
_CLASSES = (("normal", 5), ("+0", 2), ("-0", 2), ("+sub", 1), ("-sub", 1), ("+submin", 1), ("-submin", 1), ("+tiny", 1), ("-tiny", 1), ("+huge", 1), ("-huge", 1))


def _values(cls, r, n, dt):
    """n values of class `cls`."""
    fi = np.finfo(dt)
    sign = dt(-1.0) if cls[0] == "-" else dt(1.0)
    kind = cls.lstrip("+-")
    if kind == "normal":
        return (r.random(n) * 2.0 - 1.0).astype(dt)
    if kind == "0":
        return np.full(n, sign * dt(0.0), dt)
    if kind == "sub":             # k * smallest subnormal, 1 <= k < 2^mantissa bits
        k = r.integers(1, 1 << fi.nmant, n)
        return sign * (k.astype(np.float64) * float(fi.smallest_subnormal)).astype(dt)
    if kind == "submin":
        return np.full(n, sign * fi.smallest_subnormal, dt)
    if kind == "tiny":
        return np.full(n, sign * fi.tiny * dt(1.5), dt)
    assert kind == "huge", cls
    v = (np.ldexp(1.0 - r.random(n) * 0.5, -r.integers(0, 16, n)) * float(fi.max)).astype(dt)      # (max / 2^16, max]
    v[r.random(n) < 0.1] = fi.max
    return sign * v


def special_fill(shape, dtype, seed, block):
    """An array of `shape`: planes (rows in 2D) [0, n0 // 2) of the outermost axis class per cell, the others class per block of edge
    `block` (block grid anchored at the cut and at index 0 of the inner axes; the last blocks may be cut short)."""
    dt = np.dtype(dtype).type
    r = np.random.default_rng(seed)
    shape = tuple(shape)
    cut = shape[0] // 2
    names = [c for c, _ in _CLASSES]
    w = np.array([x for _, x in _CLASSES], float)
    # class index per cell: drawn per cell below the cut, per block above it
    cls = np.empty(shape, np.int64)
    cls[:cut] = r.choice(len(names), size=(cut,) + shape[1:], p=w / w.sum())
    nb = tuple(-(-n // block) for n in (shape[0] - cut,) + shape[1:])
    per_block = r.choice(len(names), size=nb, p=w / w.sum())
    idx = np.ix_(*[np.arange(n) // block for n in (shape[0] - cut,) + shape[1:]])
    cls[cut:] = per_block[idx]
    a = np.empty(shape, dt)
    for k, name in enumerate(names):
        m = cls == k
        a[m] = _values(name, r, int(m.sum()), dt)
    # inf and NaN: a fixed count each (the share of the per-cell half, rounded; at least one on grids of 200 cells a half and more: the smallest grids, whose every output reads most of the grid, get none)
    half = a[:cut].reshape(-1)
    count = int(round(INF_SHARE * half.size)) or (1 if half.size >= 200 else 0)
    if count:
        where = r.choice(half.size, 3 * count, replace=False)
        half[where[:count]] = np.inf
        half[where[count:2 * count]] = -np.inf
        half[where[2 * count:]] = np.nan
        a[:cut] = half.reshape((cut,) + shape[1:])
    return a


def _uint(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, ref):
    """True when got and ref have their NaNs in the same cells and the same bits in every other cell (so -0.0 differs from +0.0 and
    subnormals count); the whole arrays, whatever they hold."""
    assert got.shape == ref.shape and got.dtype == ref.dtype
    ng, nr = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(ng, nr) and np.array_equal(_uint(got)[~ng], _uint(ref)[~nr]))


def count_different(got, ref):
    """The number of cells same_bits objects to."""
    ng, nr = np.isnan(got), np.isnan(ref)
    return int(((ng != nr) | (~ng & ~nr & (_uint(got) != _uint(ref)))).sum())


def classes_present(a):
    """The output classes among the values of `a`."""
    a = np.asarray(a).reshape(-1)
    tiny = np.finfo(a.dtype).tiny
    with np.errstate(all="ignore"):
        mag = np.abs(a)
        found = {"normal": bool(((mag >= tiny) & np.isfinite(a)).any()), "subnormal": bool(((mag > 0) & (mag < tiny)).any()),
                 "+0.0": bool(((a == 0) & ~np.signbit(a)).any()), "-0.0": bool(((a == 0) & np.signbit(a)).any()),
                 "+inf": bool((a == np.inf).any()), "-inf": bool((a == -np.inf).any()), "nan": bool(np.isnan(a).any())}
    return {c for c in OUTPUT_CLASSES if found[c]}


def reference_conditions(outputs, halo, waive=()):
    """The two conditions on the reference's arrays after the compared launches, as (finite share, missing classes): `outputs` are the
    arrays the compared launches wrote (after two launches of the ping-pong: both).  The finite share is the smallest over them and
    must be at least 1/4; the classes are looked for in their interiors together (the second launch reads what the first one wrote,
    which is no longer block-wise) and every one of OUTPUT_CLASSES not in `waive` must be there."""
    inner = [o[tuple(slice(halo, n - halo) for n in o.shape)] for o in outputs]
    share = min(float(np.isfinite(i).mean()) for i in inner)
    present = set().union(*[classes_present(i) for i in inner])
    return share, [c for c in OUTPUT_CLASSES if c not in present and c not in waive]


# ---- the cases: single-pass kernels that __graft_entry__.build() prebuilds --------------------------------------------------------------
LAUNCHES = 2                # both directions of the ping-pong
SEEDS = (0, 1, 2)           # A, B and the source array
# The seed of a case's fill, where 0 does not put the classes asserted below among the reference's outputs: found by trying seeds on the
# reference alone.  7 x 9 x 13 under Halo 2 has 3 x 5 x 9 interior cells, 45 of them in the per-cell half.
SEED_BASE = {"edge_thin_7x9x13_fp32_s2_mixed": 1221, "edge_thin_7x9x13_fp64_s2_mixed": 633,
             "edge_thin_7x9x13_fp32_periodic_s2_modest": 46, "edge_thin_7x9x13_fp32_periodic_s2_default": 3022,
             "edge_thin_7x9x13_fp64_periodic_s2_modest": 46, "edge_thin_7x9x13_fp64_periodic_s2_default": 1487,
             "edge_min_12x12_fp32_s4_reflect_modest": 20486, "edge_min_12x12_fp32_s4_reflect_default": 31,
             "edge_min_12x12_fp32_s4_modest": 705, "edge_min_12x12_fp32_s4_default": 705}


def _edge_ids(cid):
    return cid.startswith(("thin_7x9x13", "tile_plus1", "min_"))


def gpu_cases():
    """(id, ndim, stc, options) of the GPU test: the non-temporal cases of gpu_cases.SMALL, periodic_cases.SMALL,
    boundary_cases.gpu_small_cases(), wave_cases.SMALL, source_cases.SMALL + BOTH and the thin / tile_plus1 / min edge grids of the
    three edge lists.  Options that ask for on-chip stages are left out here, and the tests assert info["stages"] == 1 of the rest."""
    import boundary_cases
    import gpu_cases as g
    import mode_fuzz_cases
    import periodic_cases
    import source_cases
    import wave_cases
    out = [("parity_" + c, n, s, o) for c, n, s, o in g.SMALL]
    out += [("periodic_" + c, n, s, o) for c, n, s, o in periodic_cases.SMALL]
    out += [("boundary_" + c, n, s, o) for c, n, s, o in boundary_cases.gpu_small_cases()]
    out += [("order2_" + c, n, s, o) for c, n, s, o in wave_cases.SMALL]
    out += [("source_" + c, n, s, o) for c, n, s, o in source_cases.SMALL + source_cases.BOTH]
    out += [("edge_" + c, n, s, o) for c, n, s, o, _ in mode_fuzz_cases.EDGE if _edge_ids(c)]
    out += [("edge_" + c, n, s, o) for c, n, s, o in boundary_cases.edge_cases() if _edge_ids(c)]
    out += [("edge_source_" + c, n, s, o) for c, n, s, o in source_cases.edge_cases() if _edge_ids(c)]
    return [c for c in out if "--temporal" not in c[3]]


# The classes a case need not show among the reference's outputs (the finite share is never waived); every other case asserts all seven.
# 3 x 3 x 3 (one interior cell) and 6 x 6 x 6 (2 x 2 x 2 interior cells under Halo 2) cannot hold the classes: every class waived.
# The other entries name the classes one by one; the two geometry variants of a grid run on different seeds, so that between them the
# grid shows every class a seed can supply there.
#   7 x 9 x 13, fully periodic under Halo 2: the wrap overwrites the ring, so the data is one period of 3 x 5 x 9 cells, its z = 2 plane
#   drawn per cell, the other two per block, and the fill's single +inf, -inf and NaN cell each lands in that plane in 45 of 351
#   draws.  Every output reads all three planes, so a zero output needs its per-cell taps zero too.  No fill among several thousand seeds tried gave signed
#   zeros and all of +inf, -inf, NaN with a quarter finite; one variant asserts the zeros (and subnormal), the other +-inf and NaN.
#   12 x 12 under Halo 4: 4 x 4 interior cells, two rows per cell and two in one block, and every output's footprint (radius 4) covers
#   all of them.  special_fill puts no inf or NaN on a grid with fewer than 200 cells in its per-cell half (one NaN would reach every
#   output), so +-inf and NaN could come from overflow alone.  Reflecting: one variant shows subnormal and both zeros (no seed tried
#   added a normal output to those), the other normal and both zeros.  Periodic: every output sums the whole period, so a zero output
#   needs all 16 cells zero, 8 of them drawn per cell; the case keeps normal and subnormal.
_ALL = OUTPUT_CLASSES
_INF_NAN = ("+inf", "-inf", "nan")
CLASS_WAIVERS = {"edge_min_333_": _ALL, "edge_min_666_": _ALL, "edge_source_min_333_": _ALL,
                 "edge_thin_7x9x13_fp32_periodic_s2_modest": _INF_NAN, "edge_thin_7x9x13_fp32_periodic_s2_default": ("+0.0", "-0.0"),
                 "edge_thin_7x9x13_fp64_periodic_s2_modest": ("-inf", "nan"), "edge_thin_7x9x13_fp64_periodic_s2_default": ("+0.0", "-0.0"),
                 "edge_min_12x12_fp32_s4_reflect_modest": ("normal",) + _INF_NAN, "edge_min_12x12_fp32_s4_reflect_default": ("subnormal",) + _INF_NAN,
                 "edge_min_12x12_fp32_s4_modest": ("+0.0", "-0.0") + _INF_NAN, "edge_min_12x12_fp32_s4_default": ("+0.0", "-0.0") + _INF_NAN}


def waived_classes(cid):
    return tuple(c for k, v in CLASS_WAIVERS.items() if cid.startswith(k) for c in v)


def step_of(opts):
    return int(opts[opts.index("--step") + 1]) if "--step" in opts else 1


def inputs(cid, spec, opts):
    """(A0, B0, F0 or None): the special fill with blocks of 2 Halo + 1 cells, a seed per array."""
    dt = np.float32 if "fp32" in opts else np.float64
    block = 2 * spec.halo + 1
    base = max([v for k, v in SEED_BASE.items() if cid.startswith(k)] or [0])
    A0, B0 = (special_fill(spec.shape, dt, base + s, block) for s in SEEDS[:2])
    return A0, B0, (special_fill(spec.shape, dt, base + SEEDS[2], block) if "--source" in opts else None)


def reference(spec, ndim, opts, A, B, F, launches=LAUNCHES):
    """The existing host reference of what the options name (options_reference.options_reference: oracle.sweep(..., contract=1),
    periodic_cases.oracle_periodic_run, boundary_cases.oracle_boundary_run, wave_cases.host_run, source_cases.host_run), unchanged and in
    place, under np.errstate(all="ignore")."""
    from options_reference import options_reference
    with np.errstate(all="ignore"):
        assert options_reference(spec, ndim, opts, A, B, F, launches) == launches
    return A, B


def assert_conditions(cid, spec, Ar, Br):
    """The finite share and the class presence, on the reference alone."""
    waive = waived_classes(cid)
    share, missing = reference_conditions((Ar, Br), spec.halo, waive)
    assert share >= 0.25, (cid, share)
    assert not missing, (cid, missing)
    return share


# ---- the emulated suite: the same cases on smaller grids (the emulator runs one fiber per lane) ----------------------------------------
def emulated_dims(stc, ndim):
    """The grid of the emulated run of a case: the edge grids as they are, every other spec cut down to a grid that still has several
    tiles and stream blocks, a partial x-edge tile, a block half several blocks deep, and the spec's own N modulo 4 (so a row is a multiple of 16 bytes, or not, as
    in the spec)."""
    import oracle
    L, M, N = oracle.Spec(stc, ndim, 1).dims
    if L * M * N <= 30000:
        return (L, M, N)
    return (23, 23, 136 + N % 4) if ndim == 3 else (1, 71, 268 + N % 4)


def emulated_stc(tmp_path, stc, ndim):
    """The stencil of `stc` on emulated_dims, written into tmp_path."""
    import os
    import oracle
    from helpers import write_stc
    spec = oracle.Spec(stc, ndim, 1)
    dims = emulated_dims(stc, ndim)
    if tuple(dims) == tuple(spec.dims):
        return stc
    path = os.path.join(str(tmp_path), os.path.basename(stc))
    write_stc(path, ndim, dims, 4, [tuple(off[3 - ndim:]) + (c,) for off, c, *_ in spec.points])
    return path


def emulated_cases():
    """The emulated sample, cut for run time (the GPU test runs every case): every fourth case of gpu_cases.SMALL, the edge grids under
    the modest geometry only, every other family whole."""
    out, parity = [], 0
    for c in gpu_cases():
        if c[0].startswith("parity_"):
            parity += 1
            if parity % 4 != 1:
                continue
        if c[0].startswith("edge_") and c[0].endswith("_default"):
            continue
        out.append(c)
    return out
