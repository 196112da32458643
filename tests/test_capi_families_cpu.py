"""Which family of launch entry points of the C ABI accepts which kind of kernel (include/drstencil_amd.h): every public launch / run /
run_timed / solve entry point of the plain, _src, _res, _fix and _ops families on the nine launch interfaces a plugin can have, with dummy
pointers.  A family's entry point accepts a kernel exactly when the plugin exports that family's symbol and the arrays go with the kernel;
everything else is -2 and launches nothing.  The table of what is accepted is written out by hand from the header.  An accepted call
would launch, so it is never made: the kernels are cross-compiled and loaded, no GPU is needed."""
import ctypes

import drstencil_amd as drs
import residual_cases as rc

SRC, RES, FIX, SCALE, COEF = 3, 4, 5, 6, 7          # dummy device addresses, one per array
# the nine interfaces: name -> (options, the arrays the kernel takes)
INTERFACES = {
    "plain": ([], {}),
    "source": (["--source"], {"src": SRC}),
    "residual": (["--residual", "max"], {"res": RES}),
    "residual_source": (["--residual", "max", "--source"], {"src": SRC, "res": RES}),
    "dirichlet": (["--dirichlet"], {"fix": FIX}),
    "dirichlet_source_residual": (["--dirichlet", "--source", "--residual", "max"], {"src": SRC, "res": RES, "fix": FIX}),
    "scale": (["--scale"], {"scale": SCALE}),
    "varcoef": (["--varcoef"], {"coef": COEF}),
    "all": (["--scale", "--varcoef", "--source", "--residual", "max", "--dirichlet"], {"src": SRC, "res": RES, "fix": FIX, "scale": SCALE, "coef": COEF}),
}
# What each kernel is accepted by, given the right arrays (include/drstencil_amd.h).  The plugin of a --source kernel exports the _src
# symbols instead of the plain ones; --residual max replaces the sweep's symbol by _res and keeps the gold one; --dirichlet exports the
# _fix pair and --scale / --varcoef the _ops pair instead of every other; a solve needs --residual max.  The _ops family takes every kernel
OPS_ALWAYS = {"launch_ops", "launch_gold_ops", "run_ops", "run_gold_ops", "run_timed_ops"}
ACCEPTED = {
    "plain": {"launch", "launch_gold", "run", "run_gold", "run_timed"},
    "source": {"launch_src", "launch_gold_src", "run_src", "run_gold_src", "run_timed_src"},
    "residual": {"launch_gold", "launch_res", "run_res", "run_timed_res", "solve", "solve_ops"},
    "residual_source": {"launch_gold_src", "launch_res", "run_res", "run_timed_res", "solve", "solve_ops"},
    "dirichlet": {"launch_fix", "launch_gold_fix", "run_fix", "run_gold_fix", "run_timed_fix"},
    "dirichlet_source_residual": {"launch_fix", "launch_gold_fix", "run_fix", "run_gold_fix", "run_timed_fix", "solve_fix", "solve_ops"},
    "scale": set(),
    "varcoef": set(),
    "all": {"solve_ops"},
}


def _block(o, size=None):
    return ctypes.byref(drs.Operands(ctypes.sizeof(drs.Operands) if size is None else size, o.get("src"), o.get("res"), o.get("fix"), o.get("scale"), o.get("coef")))


def _entries(L, ms):
    """name -> call(handle, arrays): every entry point, on in = 1, out = 2, four iterations, no warm-up; `arrays` maps src / res / fix /
    scale / coef to an address or is silent about it (NULL)."""
    s, r, x = (lambda o: o.get("src")), (lambda o: o.get("res")), (lambda o: o.get("fix"))
    return {
        "launch": lambda h, o: L.drs_kernel_launch(h, 1, 2, 0),
        "launch_gold": lambda h, o: L.drs_kernel_launch_gold(h, 1, 2, 0),
        "run": lambda h, o: L.drs_kernel_run(h, 1, 2, 4, 0, 0),
        "run_gold": lambda h, o: L.drs_kernel_run(h, 1, 2, 4, 1, 0),
        "run_timed": lambda h, o: L.drs_kernel_run_timed(h, 1, 2, 4, 0, 0, ms),
        "launch_src": lambda h, o: L.drs_kernel_launch_src(h, 1, 2, s(o), 0),
        "launch_gold_src": lambda h, o: L.drs_kernel_launch_gold_src(h, 1, 2, s(o), 0),
        "run_src": lambda h, o: L.drs_kernel_run_src(h, 1, 2, s(o), 4, 0, 0),
        "run_gold_src": lambda h, o: L.drs_kernel_run_src(h, 1, 2, s(o), 4, 1, 0),
        "run_timed_src": lambda h, o: L.drs_kernel_run_timed_src(h, 1, 2, s(o), 4, 0, 0, ms),
        "launch_res": lambda h, o: L.drs_kernel_launch_res(h, 1, 2, s(o), r(o), 0),
        "run_res": lambda h, o: L.drs_kernel_run_res(h, 1, 2, s(o), r(o), 4, 0),
        "run_timed_res": lambda h, o: L.drs_kernel_run_timed_res(h, 1, 2, s(o), r(o), 4, 0, 0, ms),
        "solve": lambda h, o, every=1: L.drs_kernel_solve(h, 1, 2, s(o), r(o), 1e-3, 8, every, 0, None, None),
        "launch_fix": lambda h, o: L.drs_kernel_launch_fix(h, 1, 2, s(o), r(o), x(o), 0),
        "launch_gold_fix": lambda h, o: L.drs_kernel_launch_gold_fix(h, 1, 2, s(o), x(o), 0),
        "run_fix": lambda h, o: L.drs_kernel_run_fix(h, 1, 2, s(o), r(o), x(o), 4, 0, 0),
        "run_gold_fix": lambda h, o: L.drs_kernel_run_fix(h, 1, 2, s(o), r(o), x(o), 4, 1, 0),
        "run_timed_fix": lambda h, o: L.drs_kernel_run_timed_fix(h, 1, 2, s(o), r(o), x(o), 4, 0, 0, ms),
        "solve_fix": lambda h, o, every=1: L.drs_kernel_solve_fix(h, 1, 2, s(o), r(o), x(o), 1e-3, 8, every, 0, None, None),
        "launch_ops": lambda h, o: L.drs_kernel_launch_ops(h, 1, 2, _block(o), 0),
        "launch_gold_ops": lambda h, o: L.drs_kernel_launch_gold_ops(h, 1, 2, _block({n: v for n, v in o.items() if n != "res"}), 0),
        "run_ops": lambda h, o: L.drs_kernel_run_ops(h, 1, 2, _block(o), 4, 0, 0),
        "run_gold_ops": lambda h, o: L.drs_kernel_run_ops(h, 1, 2, _block({n: v for n, v in o.items() if n != "res"}), 4, 1, 0),
        "run_timed_ops": lambda h, o: L.drs_kernel_run_timed_ops(h, 1, 2, _block(o), 4, 0, 0, ms),
        "solve_ops": lambda h, o, every=1: L.drs_kernel_solve_ops(h, 1, 2, _block(o), 1e-3, 8, every, 0, None, None),
    }


# the arrays an entry point has parameters for, beside those of the operand block
PARAMETERS = {"": (), "src": ("src",), "res": ("src", "res"), "fix": ("src", "res", "fix"), "ops": ("src", "res", "fix", "scale", "coef")}


def _family(name):
    return name.rsplit("_", 1)[1] if name.rsplit("_", 1)[-1] in ("src", "res", "fix", "ops") else "res" if name == "solve" else ""


def test_every_family_on_every_interface(tmp_path):
    cid, ndim, stc, opts = rc.EDGE[1]                      # 7 x 9 x 13, fp32: the smallest grid of the case modules with more than one interior cell
    L = drs.lib()
    ms = ctypes.c_float()
    entries = _entries(L, ms)
    assert sorted(entries) == sorted(set().union(OPS_ALWAYS, *ACCEPTED.values()))
    kernels = {name: drs.Kernel(list(opts) + more + [stc]) for name, (more, takes) in INTERFACES.items()}
    refused = 0
    for name, (more, takes) in INTERFACES.items():
        h = kernels[name].h
        accepted = ACCEPTED[name] | OPS_ALWAYS
        for entry, call in entries.items():
            fam = _family(entry)
            # the right arrays: what the kernel takes of the entry point's parameters -- and the family's own array in any case, so that a
            # kernel of another family is refused for its family and not for a null pointer
            right = {n: v for n, v in takes.items() if n in PARAMETERS[fam]}
            if fam in ("src", "res", "fix"):
                right[fam] = {"src": SRC, "res": RES, "fix": FIX}[fam]
            if entry not in accepted:
                assert call(h, right) == -2, (name, entry)
                refused += 1
                continue
            # accepted with the right arrays (not called: it would launch); -2 with one array missing or one too many
            gold = "gold" in entry
            for n in PARAMETERS[fam]:
                if gold and n == "res" and entry != "run_gold_fix":
                    continue                                # the gold forms take no res (drs_kernel_run_fix asks for it as its sweep does)
                wrong = dict(right)
                if n in wrong:
                    del wrong[n]
                else:
                    wrong[n] = 9
                assert call(h, wrong) == -2, (name, entry, n)
                refused += 1
            if entry.startswith("solve"):
                assert call(h, right, 0) == -2, (name, entry, "check_every_pairs < 1")
        # the operand block itself: none, a short one, a long one
        for size in (8, ctypes.sizeof(drs.Operands) + 8):
            assert L.drs_kernel_launch_ops(h, 1, 2, _block(takes, size), 0) == -2 and L.drs_kernel_run_ops(h, 1, 2, _block(takes, size), 4, 1, 0) == -2
        assert L.drs_kernel_launch_ops(h, 1, 2, None, 0) == -2 and L.drs_kernel_solve_ops(h, 1, 2, None, 1e-3, 8, 1, 0, None, None) == -2
        # a gold form of the block takes a res on a --residual max kernel and on no other
        if "res" not in takes:
            assert L.drs_kernel_launch_gold_ops(h, 1, 2, _block(dict(takes, res=RES)), 0) == -2 and L.drs_kernel_run_ops(h, 1, 2, _block(dict(takes, res=RES)), 4, 1, 0) == -2
    assert refused > 300
    # nothing was launched, so this process may still compile: a build that misses the cache succeeds (after a launch it is refused)
    assert drs.Kernel(list(opts) + [stc], cache_dir=str(tmp_path)).path.startswith(str(tmp_path))
