"""The random knobs of a shape sweep's configurations, shared by the manual sweep (tests/fuzz_shapes.py) and the fixed sample of the
test suite (tests/shape_mode_cases.py): which --dist a point set has data to reuse at, and the option list of one vector of the
tuner's space with the sweep's draws."""
import fuzz_parity as fp
from drstencil_amd.tuner import tuning as t


def legal_dists(pts, step):
    """The --dist values for which the reference finds data to reuse (drstencil.hpp:198-259): some point of the fused
    stencil has another one `dist` behind it along the outermost dimension."""
    offs = {p[:-1] for p in pts}
    fused = {tuple([0] * len(next(iter(offs))))}
    for _ in range(step):
        fused = {tuple(a + b for a, b in zip(f, o)) for f in fused for o in offs}
    span = max(f[0] for f in fused) - min(f[0] for f in fused)
    return [d for d in range(1, span + 1) if any((f[0] - d,) + f[1:] in fused for f in fused)]


def config_options(rnd, v, ndim, h, pts, mixed, dists):
    """The option list of space vector `v` for the shape `pts` with the sweep's random knobs drawn from `rnd` (--dist inside and
    outside the shape's legal set, the memory path, staging, round 3's and round 4's emission knobs), or None for a temporal pipeline on
    a mixed-sign shape.  dists: a cache of legal_dists by step."""
    cl = t.cfgToCommandLine(v).split()
    if "--temporal" in cl and mixed:
        return None                      # a relative bar means nothing where the sum cancels
    r = rnd.random()
    i = cl.index("--dist")
    legal = dists.setdefault(v[0], legal_dists(pts, v[0]))
    if r < 0.2:                      # the reference's range, (step-1)*order .. step*order (tuning.py:20): refused ("No data to reuse") or right
        cl[i + 1] = str(rnd.randint(max(1, (v[0] - 1) * h), v[0] * h))
    elif r < 0.4 and legal:          # a distance this shape has data to reuse at
        cl[i + 1] = str(rnd.choice(legal))
    elif r < 0.45:                   # anything: must be refused or right
        cl[i + 1] = str(rnd.randint(1, 2 * v[0] * h + 1))
    elif r < 0.6:                    # the default, (high - low) / 2
        del cl[i:i + 2]
    if ndim == 2 and rnd.random() < 0.5:
        cl.append("--streaming")
    if "--prefetch-depth" in cl:
        cl[cl.index("--prefetch-depth") + 1] = str(rnd.choice([1, 2, 3, 4]))
    if "--schedule" not in cl and rnd.random() < 0.6:
        cl[cl.index("--merge-forward") + 1] = str(rnd.choice([0, 2, 3, 100]))
    if rnd.random() < 0.2:
        cl += ["--uniform-loads", str(rnd.choice([1, 2]))]
    if rnd.random() < 0.2:
        cl += ["--store-mask", "buffer"]
    if rnd.random() < 0.25 and "--temporal" not in cl and "--cyclic-merge-y" not in cl and (ndim == 3 or "--streaming" in cl):
        cl += ["--stage", "dma"]
    if rnd.random() < 0.2:
        cl += ["--defer-stores", "1"]
    if fp.ROUND3:
        fp.round3_knobs(rnd, cl)
        fp.round4_knobs(rnd, cl)
        if "--skew" in cl and ndim == 2 and "--streaming" not in cl:
            del cl[cl.index("--skew"):cl.index("--skew") + 2]
    return cl
