"""The GPU sample of the mode fuzz (tests/test_mode_fuzz_gpu.py): random tuner-space configurations with --boundary periodic and / or
--time-order 2 (tests/fuzz_parity.py: make_jobs(n, seed, mode)), and explicit edge grids of the two options.  Every kernel is prebuilt
by __graft_entry__.build() beside the sampled parity fuzz, so that the GPU box finds it -- or the compiler's resource report that makes
the runtime refuse it -- in drstencil_amd/_kcache and no test starts hipcc.

Refusals are decided when build() compiles (the runtime refuses kernels that spill to scratch or spill scalar registers, the generator
rejects an LDS demand beyond the limit or a tile that does not cover the halo), so they are known before any GPU run.  build() printed
for this sample, cross-compiling for gfx950:
    mode fuzz periodic: 18 kernels built, 2 refused
    mode fuzz order2: 17 kernels built, 3 refused
    mode fuzz order2_periodic: 18 kernels built, 2 refused
(2 for scratch spills, 4 for LDS-DMA staging on a row length that is no multiple of the 16-byte vector, 1 for an LDS demand beyond
160 KiB).  The test asserts at least three quarters of each mode checked (MIN_CHECKED)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STC = os.path.join(ROOT, "tests", "stc")
PERIODIC = ["--boundary", "periodic"]
ORDER2 = ["--time-order", "2"]

MODES = ("periodic", "order2", "order2_periodic")
SAMPLE = (20, 4)            # (configurations per mode, seed)
MIN_CHECKED = 15            # three quarters of a mode's sample


def stc(name):
    return os.path.join(STC, name + ".stc")


def sample_jobs(mode):
    import fuzz_parity
    return fuzz_parity.make_jobs(SAMPLE[0], SAMPLE[1], mode)


# ---- edge grids -------------------------------------------------------------------------------------------------------------------
# Two geometries each: a modest one (16-lane rows, 8-row tiles, stream blocks of 4 planes; 2D tiles tall enough for the halo) and the
# generator's default.  (id, ndim, stc, options, mode)
_G3 = ["--bx", "16", "--by", "4", "--block-merge-y", "2", "--sn", "4"]
_G2 = ["--bx", "16", "--by", "4", "--block-merge-y", "4"]           # 16 rows: a step-4 tile keeps 8 of them
_W256 = ["--bx", "64", "--by", "4", "--block-merge-x", "4", "--block-merge-y", "2", "--sn", "4"]     # 256 columns per tile: 4 points per lane

EDGE = []


def _edge(cid, ndim, name, mode, opts, geometries):
    extra = {"periodic": PERIODIC, "order2": ORDER2, "order2_periodic": ORDER2 + PERIODIC}[mode]
    for gid, g in geometries:
        EDGE.append(("%s_%s" % (cid, gid), ndim, stc(name), (["--3d"] if ndim == 3 else []) + opts + g + extra, mode))


_BOTH3 = [("modest", _G3), ("default", [])]
# the smallest legal periodic grids, every dimension exactly 3 Halo: the period is the ring's width, every ghost is one period away
# (edge3_min_h1's coefficients sum to 0.9, not 1: on its single interior cell every tap reads the same value, and a sum of 1 would make
# a launch the identity, which a kernel that computes nothing also is)
_edge("min_333_fp32_s1_elem", 3, "edge3_min_h1", "periodic", ["--dtype", "fp32"], _BOTH3)                      # N * 4 % 16 != 0: element path
_edge("min_666_fp64_s2_vec", 3, "edge3_min_h2", "periodic", ["--dtype", "fp64", "--step", "2"], _BOTH3)        # ghosts of both sides inside one 16-byte vector
_edge("min_12x12_fp32_s4", 2, "edge2_min_h4", "periodic", ["--dtype", "fp32", "--step", "4"], [("modest", _G2), ("default", [])])
# ... the same 3 x 3 x 3 grid, order 2: one interior cell whose every tap is its own image
_edge("min_333_fp32_order2", 3, "edge3_min_h1", "order2_periodic", ["--dtype", "fp32"], _BOTH3)
_edge("min_333_fp64_order2", 3, "edge3_min_h1", "order2_periodic", ["--dtype", "fp64"], _BOTH3)
# narrower than a wavefront's row, a tile and (fp32: 13 * 4 % 16 != 0) a vector row in every direction, odd N: one partial tile; one
# stream block under the default geometry, two under the modest one
_edge("thin_7x9x13_fp32_order2", 3, "edge3_thin", "order2", ["--dtype", "fp32"], _BOTH3)
_edge("thin_7x9x13_fp64_order2", 3, "edge3_thin", "order2", ["--dtype", "fp64"], _BOTH3)
_edge("thin_7x9x13_fp32_periodic_s2", 3, "edge3_thin", "periodic", ["--dtype", "fp32", "--step", "2"], _BOTH3)
_edge("thin_7x9x13_fp64_periodic_s2", 3, "edge3_thin", "periodic", ["--dtype", "fp64", "--step", "2"], _BOTH3)
# interior width in x = whole tiles plus ONE column (N = 2 Halo + 256 + 1; the default fp32 tile owns 128 columns): the last tile
# stores, and loads an old value for, a single column
_TILES = [("w256", _W256), ("default", [])]
_edge("tile_plus1_fp32_order2_buffer", 3, "edge3_tile_plus1", "order2", ["--dtype", "fp32", "--store-mask", "buffer"], _TILES)
_edge("tile_plus1_fp32_order2", 3, "edge3_tile_plus1", "order2", ["--dtype", "fp32"], _TILES)

# the fp64 minimum grid also runs against np.roll (no oracle involved), within 1e-12
ROLL_IDS = ("min_666_fp64_s2_vec_modest", "min_666_fp64_s2_vec_default")


def edge_build_args():
    return [c[3] + [c[2]] for c in EDGE]
