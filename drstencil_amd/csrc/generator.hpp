// generator.hpp -- the `drstencil` command as a function: argv -> (messages, exit code,
// emitted source).  Option surface, defaults, messages and exit codes follow the
// reference's main.cpp:10-280 (hand-rolled scan 118-230: the last argument is always the
// .stc; a value-taking flag in the second-to-last slot is "Illegal input." exit 255; an
// unknown flag is "Illegal input." exit 0; `-o` without a value is ignored), plus
// additive MI355X options that the reference does not have.
#pragma once
#include <algorithm>
#include <cmath>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "emit_hip.hpp"
#include "planner.hpp"
#include "stencil_ir.hpp"
#include "tuned_defaults.hpp"

namespace drs {

// ---- tuner -> generator feedback (round 4; reference: benchmarks/3d7pt_star/tuning.py:125-131 ends with the best configuration in
// duration.log).  tuned_defaults.hpp is generated from drstencil_amd/tuned_defaults.tsv, which `tuning.py --write-defaults` maintains.
inline unsigned tuned_shape_hash(const CoefTable &base) {          // FNV-1a over "k,j,i;" of the one-step stencil's offsets in map order
    unsigned h = 0x811c9dc5u;
    for (auto &e : base.v) {
        char b[64];
        snprintf(b, sizeof b, "%d,%d,%d;", e.first.k, e.first.j, e.first.i);
        for (const char *c = b; *c; c++) h = (h ^ (unsigned char)*c) * 0x01000193u;
    }
    return h;
}
// the row of this problem class whose N is nearest in log2 (within a factor of sqrt 2), or nullptr
inline const TunedDefault *tuned_lookup(const char *mode, unsigned shape, int step, const std::string &dtype, int temporal, int N) {
    const TunedDefault *best = nullptr;
    double bestd = 0.0;
    for (int i = 0; i < kTunedDefaultsCount; i++) {
        const TunedDefault &r = kTunedDefaults[i];
        if (std::string(r.mode) != mode || r.shape != shape || r.step != step || dtype != r.dtype || r.temporal != temporal || N <= 0) continue;
        const double d = std::fabs(std::log2((double)N / (double)r.N));
        if (d <= 0.5 + 1e-9 && (!best || d < bestd)) { best = &r; bestd = d; }
    }
    return best;
}

struct GenResult {
    int exit_code = 0;
    std::string messages;   // what the command prints on stdout
    std::string source;     // emitted HIP source (empty when nothing was emitted)
    std::string out_name;
    bool emitted = false;
    Stencil st;
    KernelPlan plan;        // as make_plan() returned it: nobody writes to it afterwards
    std::string error;      // non-empty: why the configuration is invalid (the planner's reason, the schedule's or the generator's own)
    GenOptions opt;
    std::string notes;        // what the command prints on STDERR: remarks the reference has no counterpart for on a reference command line (stdout stays the reference's)
    std::string tuned_from;   // non-empty: the geometry / emission options came from the tuned-defaults table (this row's option string)
};

inline const char *help_text() {
    return R"(
    Generate data-reusing stencil kernels for AMD Instinct MI355X (gfx950, HIP).

    Usage: drstencil [options] <input_stcfile>
Options:

-o <file>               Specify the name of the output HIP source file.
                        (out.cu by default)

--3d                    Choose 3D mode.

--step <num>            Specify the number of time steps to fuse the stencil.
                        (step_num = 1 by default)

--dist <num>            Specify the number of the distance between points for data-reuse.

--streaming             Apply streaming optimization (2D; 3D always streams).

--bx <num>              Specify the workgroup size bx (lanes along x; 64 = one wavefront).

--by <num>              Specify the workgroup size by (rows of lanes along y).

--sn <num>              Specify the length of stream block sn.

--stream-unroll <num>   Specify the (minimum) unroll factor of the streaming loop.
                        (stream_unroll = 4 by default)

--block-merge-x <num>   Specify the number of contiguous points per lane along dimension x.

--block-merge-y <num>   Specify the number of adjacent rows per lane along dimension y.

--cyclic-merge-x <num>  Specify the number of points per lane along dimension x, bx columns apart.

--cyclic-merge-y <num>  Specify the number of rows per lane along dimension y, by rows apart.

--prefetch              Prefetch the next plane into registers to hide the transfer latency.

--merge-forward <num>   Specify the threshold for whether to merge the forward_j or forward_i into backward.
                        (merge_forward = 5 by default)

--check                 Check the correctness of the generated code against the gold kernel.

--gold                  Accepted for compatibility (no effect).

MI355X options:

--dtype <fp32|fp64>     Element type (fp64 by default, as the reference).
--boundary <fixed|periodic|reflect>  The boundary treatment of every axis.  fixed (default): the ring of width Halo (= step * order)
                        around the interior is input that no launch writes (the reference's semantics).  periodic: the interior is
                        a periodic domain of period dim - 2 * Halo in every dimension (so the period depends on --step) and the ring
                        holds its ghost copies: the ghost at x takes the value at x + P (x < Halo) or x - P (x >= dim - Halo), each
                        coordinate wrapped on its own.  reflect: zero-flux (insulated / rigid) walls on the faces between ring and
                        interior: the ghost at distance d outside a face takes the interior cell at distance d - 1 inside it (x <
                        Halo takes 2 Halo - 1 - x, x >= dim - Halo takes 2 (dim - Halo) - 1 - x; numpy's pad mode "symmetric").  Every
                        launch (in -> out) first refills in's ring from in's interior -- it OVERWRITES the input array's ring on
                        the non-fixed axes -- then sweeps as with fixed; out's ring is not touched.  A non-fixed axis needs a
                        dimension >= 3 * Halo; not with --gpus N > 1 or --pair-launch 1.  A fused --step n launch applies S^n to
                        the mirrored extension, which is n mirrored one-step updates only for a stencil that is symmetric along
                        every reflecting axis (a note says so otherwise).
--boundary-x <fixed|periodic|reflect>  The boundary treatment of the x axis alone, overriding --boundary there wherever it stands on the
                        line (a channel: --boundary periodic --boundary-z reflect).  A ring cell is refilled iff one of its
                        coordinates lies in the ring of a non-fixed axis; its source has every coordinate mapped on its own, fixed
                        axes unchanged.  Three equal per-axis values are --boundary <value>.
--boundary-y <fixed|periodic|reflect>  The same for the y axis.
--boundary-z <fixed|periodic|reflect>  The same for the z axis (only fixed in 2D).
--time-order <1|2>      1 (default): out = S(in), a first-order update.  2: out = S(in) - out_old on the interior, the leapfrog
                        update of a second-order equation (wave equation: u(t+1) = S(u(t)) - u(t-1), the factor 2 of 2u folded
                        into the centre coefficient).  The ping-pong loop k(A,B); k(B,A) is then leapfrog as it stands: the
                        OUTPUT array's interior is input too (its ring is neither read nor written).  S(in) is the same FMA chain,
                        rounded once; the subtraction is one more rounded operation.  Needs --step 1; not with --temporal,
                        --gpus N > 1 or --pair-launch 1.
--source                A per-cell source term: a launch takes a third array src of the grid's shape and dtype and computes
                        out = S(in) + src on the interior (Jacobi for Poisson's equation: u <- avg(u) + h^2/2d f; a heat source; a
                        forcing of the wave equation).  With --time-order 2: out = (S(in) - out_old) + src.  S(in) is the same FMA
                        chain, rounded once; the addition is one more rounded operation.  src is read in the interior only and never
                        written; it must not overlap out; the same src goes to every launch of the ping-pong loop.  The kernel is
                        dr_<name>(in, out, src) and the plugin exports drs_plugin_launch_src / drs_plugin_launch_gold_src.  Needs
                        --step 1; not with --temporal, --gpus N > 1 or --pair-launch 1.
--residual <max>        A launch also produces the convergence residual of the sweep it has just made: one scalar of the grid's dtype,
                        r = max over the interior of |out - in|, where out is the value the launch stores (after - out_old and + src where those
                        are on) and out - in is one rounded subtraction.  The maximum propagates NaN: r is NaN if any term is.  It is fused
                        into the sweep: every stored value meets the input's value of its cell in registers, each workgroup writes one partial
                        and a second, one-workgroup kernel folds them -- no atomics, bit-identical to numpy's max(abs(out - in)) on every
                        schedule.  The launch takes one more array d_res of residual_elems = 1 + grid elements (kernel info), written whole by
                        every launch: d_res[0] is r.  The stored arrays are those of the same command without the option.  The plugin exports
                        drs_plugin_launch_res(in, out, src, res) instead of the sweep's launch entry point.  With a fused --step n the
                        residual is max |S^n(in) - in|.  Only max; not with --temporal, --gpus N > 1 or --pair-launch 1.
--dirichlet             Held cells inside the domain: a launch takes one more array fix of the grid's shape and dtype and stores, at every
                        interior point p, out[p] = (fix[p] != fix[p]) ? v : fix[p], where v is the value the same command without the option
                        would store (S(in), then - out_old with --time-order 2, then + src with --source).  A cell whose fix is NaN (any sign,
                        any payload) is free; every other cell is held and receives fix[p] bit for bit (+-0, subnormals and +-inf included).
                        A select, never arithmetic: a held cell stores fix[p] whatever v is.  S(in) reads in as it is, so write fix into the
                        input first (and into the output with --time-order 2) if the first launch is to see the held values.  fix is read
                        in the interior only and never written; it must not overlap out; the same fix goes to every launch.  --residual max
                        sees the selected value.  The kernel is dr_<name>(in, out, [src,] [res,] fix) and the plugin exports
                        drs_plugin_launch_fix / drs_plugin_launch_gold_fix instead of the other launch entry points.  Needs --step 1; not with
                        --temporal, --gpus N > 1 or --pair-launch 1.
--scale                 A per-cell factor: a launch takes one more array w of the grid's shape and dtype and computes, at every interior
                        point p, v = w[p] * S(in)[p] -- one rounded multiplication on the unchanged FMA chain -- in front of - out_old
                        (--time-order 2), + src (--source) and the --dirichlet select.  w is read in the interior only and never written; it
                        must not overlap out; the same w goes to every launch.  With w = 1 everywhere the stored bits are those of the same
                        command without the option.  The kernel is dr_<name>(in, out, [src,] [res,] [fix,] w) and the plugin exports
                        drs_plugin_launch_ops / drs_plugin_launch_gold_ops instead of the other launch entry points.  Needs --step 1; not
                        with --temporal, --gpus N > 1 or --pair-launch 1.
--scale-centre <c>      With --scale: v = C * in[p] + w[p] * S(in)[p], a rounded product and a rounded sum behind the multiplication by w,
                        nothing contracted.  C is c as a coefficient of the .stc is written (six digits, cast to the dtype); c is a finite
                        real, default 0 (no centre term).  With S = L, a stencil whose taps sum to 0:
                          heterogeneous diffusion  u' = u + k*L(u)            --scale --scale-centre 1, w = kappa*dt/h^2
                          wave, velocity model     u' = 2u + v*L(u) - u_old   --scale --scale-centre 2 --time-order 2, w = v^2*dt^2/h^2
                          Jacobi, variable diagonal u' = A(u)/d + f/d          --scale --source, S the off-diagonal average, w = 1/diag, src = f/diag
--varcoef               One coefficient array per tap: a launch takes one more array coef of the grid's dtype and shape (T, L, M, N) -- (T, M, N)
                        in 2D --, T the taps of the one-step stencil in gold order (the kernel info lists them: "coef_taps"), and computes
                        at every interior point p  v = a_0[p] * in[p + d_0];  v = fma(a_t[p], in[p + d_t], v), t = 1 .. T-1  -- the
                        unchanged FMA chain, the array value in the constant's place -- in front of the other options' operations.  The
                        .stc constants define the shape and the tap order only.  Each of the T grids is read in its interior only, each
                        value reaching only its own cell and tap; coef is never written and must not overlap out.  With a_t = the
                        constant as it is written everywhere, the stored bits are those of the same command without the option.  The
                        kernel is dr_<name>(in, out, [src,] [res,] [fix,] [w,] coef) and the plugin exports drs_plugin_launch_ops /
                        drs_plugin_launch_gold_ops with one more pointer.  Needs --step 1; not with --temporal, --gpus N > 1,
                        --pair-launch 1, --coef or --pack 1.  Without a geometry option the tuner's row is stepped down
                        until the T coefficient values per point fit the register file (rows per lane, then points per row, then --by).
                          heterogeneous diffusion  u' = u + dt*div(k grad u)   a_t = dt*k(face t)/h^2, a_centre = 1 - their sum
                          anisotropic operator     u' = sum a_t(p) u(p + d_t)  a_t from the local tensor (rotated, stretched)
                          Jacobi, stencil-form A   u' = (f - R u)/diag         --varcoef --source, a_t = -A_t/diag, a_centre = 0, src = f/diag
--xrim <lds|dpp>        x halo inside a wavefront by DPP wave shifts (default) or through LDS.
--schedule <scatter|reuse|window>  How reuse along the streamed dimension is split between source planes kept on chip and
                        partial sums carried in VGPRs (results never depend on it):
                        scatter (default without --dist): nothing retained, every arriving plane adds its taps to the partial
                        sums of all output planes in flight;
                        reuse (default with --dist d): the reference's split for that dist -- `Range` source planes stay
                        resident in register windows, partial sums are carried over the remaining planes; a retained
                        plane's in-plane neighbours are kept in registers when that plane has at least --merge-forward
                        in-plane taps, else re-read from LDS when they are due;
                        window: every contributing plane resident, nothing carried.
--order <taps|rows>     Emission order of a plane's FMAs (scatter schedule; results never depend on it).  taps (default): one
                        chain per partial sum, the plane's whole rim window read up front.  rows: the arriving plane is
                        consumed one source row at a time, each row's tap groups fenced from the next (sched_barrier), so
                        that the compiler cannot stretch every row's reads over the whole plane (register pressure).
--pack <0|1>            With --order rows, fp32: two adjacent x points per v_pk_fma_f32 (bit-identical results; default 1).
--pin <0|1>             Pass every partial sum through an empty asm statement where it is updated, so that the compiler cannot
                        sink the FMA chains of the unrolled streaming loop down to the store (which keeps `Range` planes of
                        source windows alive instead of the sums; default: 1 with --order rows, else 0).
--rot-mod <n>           Scatter schedule: the partial sums rotate through n >= Range register sets (default Range).  The streaming
                        loop is unrolled by lcm(n, LDS slots, prefetch sets): e.g. Range 7 -> 14 plane bodies, --rot-mod 8 -> 8
                        (code size; the instruction cache holds 64 KB).
--row-fence <mask>      sched_barrier mask between row groups (0 default: nothing crosses; -1: no fence).
--gpus <N>              N > 1: the emitted program's main() runs the spec slab-decomposed over N GPUs of one node (z slabs in 3D, y slabs in 2D): it
                        forks one rank process per GPU before any HIP call and drives the C ABI's drs_slab_* entry points (RCCL send/recv of the
                        halo planes, overlapped with the interior sweep).  Link it with -ldrstencil_amd; DRS_SLAB_REHEARSE=r/N runs rank r alone
                        on one GPU.  The kernels in the file (and its use as a plugin) are unchanged.
--out-skew <MiB>        Placement of the output array relative to the input array: (out - in) mod 64 MiB.  A z-streaming kernel reads a few
                        planes ahead of the plane it writes; when its writes land, modulo 64 MiB, 8-16 MiB behind its read front the launch
                        takes up to 14 % longer on MI355X (profiles/r03_probe_skew4.log).  Default: chosen from the kernel's read-ahead
                        distance (32 or 0).  The emitted program allocates both arrays in one arena accordingly; callers of the C ABI
                        read the recommendation from the kernel info (out_skew_bytes, placement_period_bytes).  Results never depend on it.
--zigzag <0|1>          1: a launch whose output array lies below its input array (every second launch of the reference's ping-pong loop)
                        walks its stream blocks in reverse order and so begins on the planes the previous launch wrote last.
--coef <lit|sgpr|vgpr>  fp32: coefficients as 32-bit literals of every FMA (lit, default) or held in scalar registers (sgpr: 4-byte
                        instead of 8-byte FMAs -- code size and instruction fetch of the fused multi-step kernels; same results).
--temporal <0|1|force>  With --step n > 1: run the one-step stencil n times on chip (temporal blocking,
                        intermediate planes never leave the CU) instead of the fused stencil.  On-chip stages
                        re-associate the fused sum: 1 emits them only where the estimated drift from the reference's
                        fused arithmetic stays within 1e-6 relative (fp32; 1e-12 fp64) for the spec's `iterations`
                        and emits the fused kernel otherwise (a note says so); force emits them regardless.
--skew <0|1|2>          Temporal pipelines of streaming kernels: 1 = stage t consumes what stage t-1 completed one iteration EARLIER, so the
                        stages of an iteration are independent and share two barriers instead of one write/barrier/read round per stage;
                        2 = also double-buffers the intermediate planes' LDS slots (compact, no pads), so completed planes are written
                        during the compute phase instead of in a burst between the two barriers.
--tuned-defaults <0|1>  1 (default): a command line without any geometry / emission option takes them from the tuner's table for
                        this stencil shape, step, dtype and grid size (drstencil_amd/tuned_defaults.tsv), when it has a row.
--prefetch-depth <n>    With --prefetch: planes in flight ahead of the one being summed (n+1 register sets; default 3 (fp32) /
                        2 (fp64) for fused multi-step 3D kernels, else 1).
--pair-launch <0|1>     Also emit dr2_<name>(in0, out0, in1, out1): the same sweep over two buffer pairs in one launch.
--exact-y <0|1>         1 (default for single-stage kernels): the y halo rows of the source plane are fetched by the halo loader
                        lanes, so every tile row is owned; 0: overlapped tiles (tile rows include the halo).
--uniform-loads <0|1|2> With --prefetch: 0 (default) plane loads under `if (more planes)`; 1 issued unconditionally (past the
                        block's last plane they re-read it); 2 unconditionally through a buffer window that closes past it.
                        1 and 2 leave no vector-memory instruction under a branch: exact s_waitcnt vmcnt(N) pipelining.
--store-mask <branch|buffer>  branch (default): guarded global stores; buffer: buffer stores whose per-lane offset is out of
                        range where the lane must not store (no branch).
--stage <reg|dma>       How an arriving plane reaches LDS in streaming kernels: reg (default) = global loads into VGPRs
                        (software prefetch) + LDS writes; dma = LDS-DMA (global_load_lds_dwordx4) straight into the plane's
                        LDS slot, one plane ahead, no prefetch registers (16-byte vectors, block y merging, one stage).
--loader-waves <n>      With --stage dma: n extra wavefronts per workgroup only request planes by LDS-DMA, --prefetch-depth planes
                        ahead into a ring of LDS slots, counting their own vmcnt; the bx*by consumer lanes never issue a load.
--defer-stores <0|1>    Hold a completed output plane in registers and store it one plane later, right after the next
                        plane's loads were issued (its write latency runs under that plane's work).
--drain <0|1|2>         s_waitcnt vmcnt(0) before every plane's prefetch loads (1) or before its LDS staging (2).
--cc-opt <flag>         Extra hipcc flag for this kernel (repeatable), e.g. --cc-opt -fno-slp-vectorize.
--exact-x <0|1>         1 (default): the x halo columns are fetched by the halo loader lanes; 0: overlapped tiles in x (the
                        tile's outermost lanes load them with the row and own nothing, e.g. --bx 34: 136 columns own 128).
--clamp-loads <0|1>     1 (default): branch-free loads -- lanes outside the grid read the plane origin (their
                        values never reach a stored output); 0: loads under per-lane guards.
--halo-spread <0|1>     Spread the halo loader tasks over all wavefronts (default 0: the first lanes take them).
--xedge-select <0|1>    With --xrim dpp: wavefront-edge lanes pick the LDS value by select (1) or branch (0, default).
--lazy-rims <0|1>       Read LDS rims when first needed (1) or when a plane arrives (0).
--xcd-remap <0|1|2>     workgroup to tile mapping: 0 dispatch order, 1 contiguous chunk of tiles
                        per XCD, 2 one x-y band per XCD with all XCDs on the same stream block
                        (default: 2 for 3D, 0 for 2D); 3 = like 2 with --zgroup <n> successive stream
                        blocks of a tile taken by consecutive workgroups; 4 = units of 32 consecutive tiles of one
                        stream block (the CUs of an XCD) dealt round-robin to the XCDs: neighbouring tiles run
                        together on one XCD and share their halo reads in its L2; 5 = chunks of --xcd-chunk <n> (4)
                        consecutive tiles per XCD and round (x neighbours share the lines of their x halos), one front.
--nt-store <0|1>        Non-temporal stores of the output (1 by default).
--nt-load <0|1>         Non-temporal loads of the input.
--waves-per-eu <num>    Second argument of __launch_bounds__.
--lds-pad <num>         Extra elements of padding per LDS row.
--ref-defaults          Keep the reference's 16x16x16 geometry defaults.

--help  (-h)            Print this help information on this tool.
        )";
}

// ---- the command's options, one row each: the spelling, where the value goes in GenOptions and the `*_set` marker it raises.  The
// target's type is the kind: a bool is a flag (SET1: a flag that sets an int to 1); an int takes atoi of the next word; a string takes
// the next word, from `pick` if given (checked after the scan); a setter takes it at once and rejects a bad value where the scan meets
// it.  NAMES: the option names the problem or the artefact; every other option is a tuning choice and switches the tuned-defaults
// table off.  LOCAL: kept out of the slab host's options (GenOptions::slab_args).  HIDDEN: not in help_text(), which is written by hand
// (tests/test_cli_and_ir.py holds the two together).
enum : unsigned { NAMES = 1, LOCAL = 2, HIDDEN = 4, SET1 = 8 };
using Setter = bool (*)(GenOptions &, const std::string &);
struct Opt {
    const char *name;
    unsigned attr = 0;
    bool GenOptions::*b = nullptr;
    int GenOptions::*i = nullptr;
    std::string GenOptions::*s = nullptr;
    const char *pick = nullptr;   // the values a string accepts, space-separated
    Setter put = nullptr;
    bool GenOptions::*mark = nullptr;
    constexpr Opt(const char *n, bool GenOptions::*t, unsigned a = 0) : name(n), attr(a), b(t) {}
    constexpr Opt(const char *n, int GenOptions::*t, unsigned a = 0, bool GenOptions::*m = nullptr) : name(n), attr(a), i(t), mark(m) {}
    constexpr Opt(const char *n, std::string GenOptions::*t, const char *p, unsigned a = 0, bool GenOptions::*m = nullptr)
        : name(n), attr(a), s(t), pick(p), mark(m) {}
    constexpr Opt(const char *n, Setter f, unsigned a = 0) : name(n), attr(a), put(f) {}
};
inline bool put_coef(GenOptions &o, const std::string &v) {
    const int c = v == "lit" ? 0 : v == "sgpr" ? 1 : v == "vgpr" ? 2 : -1;
    if (c >= 0) o.coef_sgpr = c;
    o.coef_set = true;
    return c >= 0;
}
inline bool put_temporal(GenOptions &o, const std::string &v) {
    const int t = v == "0" ? 0 : v == "1" ? 1 : (v == "2" || v == "force") ? 2 : -1;
    if (t >= 0) o.temporal = t;
    return t >= 0;
}
// --scale-centre <c>: a finite real, the whole word
inline bool put_scale_centre(GenOptions &o, const std::string &v) {
    char *end = nullptr;
    const double c = strtod(v.c_str(), &end);
    if (v.empty() || *end || !std::isfinite(c)) return false;
    o.scale_centre = c;
    o.scale_centre_set = true;
    return true;
}
inline bool put_cc_opt(GenOptions &o, const std::string &v) { o.cc_opts.push_back(v); return true; }

inline constexpr Opt kOptions[] = {
    // the reference's options (main.cpp:118-230)
    {"-o", &GenOptions::out_name, nullptr, NAMES | LOCAL, &GenOptions::out_set}, {"--3d", &GenOptions::is3d, NAMES},
    {"--step", &GenOptions::step, NAMES}, {"--dist", &GenOptions::dist, NAMES}, {"--streaming", &GenOptions::streaming, NAMES},
    {"--bx", &GenOptions::bx, 0, &GenOptions::bx_set}, {"--by", &GenOptions::by, 0, &GenOptions::by_set}, {"--sn", &GenOptions::sn, 0, &GenOptions::sn_set},
    {"--block-merge-x", &GenOptions::bmx, 0, &GenOptions::mx_set}, {"--cyclic-merge-x", &GenOptions::cmx, 0, &GenOptions::mx_set},
    {"--block-merge-y", &GenOptions::bmy, 0, &GenOptions::my_set}, {"--cyclic-merge-y", &GenOptions::cmy, 0, &GenOptions::my_set},
    {"--stream-unroll", &GenOptions::stream_unroll}, {"--prefetch", &GenOptions::prefetch}, {"--merge-forward", &GenOptions::merge_forward},
    {"--check", &GenOptions::check, NAMES | LOCAL}, {"--gold", &GenOptions::gold, NAMES | LOCAL},
    // additive MI355X options
    {"--dtype", &GenOptions::dtype, "fp32 fp64", NAMES}, {"--boundary", &GenOptions::boundary, "fixed periodic reflect", NAMES},
    {"--boundary-x", &GenOptions::boundary_x, "fixed periodic reflect", NAMES, &GenOptions::boundary_x_set},
    {"--boundary-y", &GenOptions::boundary_y, "fixed periodic reflect", NAMES, &GenOptions::boundary_y_set},
    {"--boundary-z", &GenOptions::boundary_z, "fixed periodic reflect", NAMES, &GenOptions::boundary_z_set},
    {"--time-order", &GenOptions::time_order, NAMES}, {"--source", &GenOptions::source, NAMES},
    {"--residual", &GenOptions::residual, "max", NAMES, &GenOptions::residual_set}, {"--dirichlet", &GenOptions::dirichlet, NAMES},
    {"--scale", &GenOptions::scale, NAMES}, {"--scale-centre", put_scale_centre, NAMES},
    {"--varcoef", &GenOptions::varcoef, NAMES},
    {"--gpus", &GenOptions::gpus, NAMES | LOCAL}, {"--pair-launch", &GenOptions::pair_launch, NAMES}, {"--temporal", put_temporal, NAMES},
    {"--out-skew", &GenOptions::out_skew, NAMES}, {"--tuned-defaults", &GenOptions::tuned_defaults, NAMES},
    {"--schedule", &GenOptions::schedule, "scatter reuse window", 0, &GenOptions::schedule_set},
    {"--order", &GenOptions::order, "taps rows", 0, &GenOptions::order_set}, {"--xrim", &GenOptions::xrim, "lds dpp"},
    {"--stage", &GenOptions::stage, "reg dma"}, {"--store-mask", &GenOptions::store_mask, "branch buffer"},
    {"--coef", put_coef}, {"--cc-opt", put_cc_opt}, {"--ref-defaults", &GenOptions::ref_defaults, SET1},
    {"--pack", &GenOptions::pack}, {"--pin", &GenOptions::pin}, {"--row-fence", &GenOptions::row_fence}, {"--rot-mod", &GenOptions::rot_mod},
    {"--skew", &GenOptions::skew}, {"--loader-waves", &GenOptions::loader_waves}, {"--prefetch-depth", &GenOptions::prefetch_depth},
    {"--exact-y", &GenOptions::exact_y}, {"--exact-x", &GenOptions::exact_x}, {"--xedge-select", &GenOptions::xedge_select},
    {"--clamp-loads", &GenOptions::clamp_loads}, {"--halo-spread", &GenOptions::halo_spread}, {"--zigzag", &GenOptions::zigzag},
    {"--defer-stores", &GenOptions::defer_stores}, {"--drain", &GenOptions::drain}, {"--uniform-loads", &GenOptions::uniform_loads},
    {"--lazy-rims", &GenOptions::lazy_rims}, {"--xcd-remap", &GenOptions::xcd_remap}, {"--nt-store", &GenOptions::nt_store},
    {"--nt-load", &GenOptions::nt_load}, {"--waves-per-eu", &GenOptions::waves_per_eu}, {"--lds-pad", &GenOptions::lds_pad},
    {"--zgroup", &GenOptions::zgroup, HIDDEN}, {"--xcd-chunk", &GenOptions::xcd_chunk, HIDDEN}, {"--prefetch-auto", &GenOptions::prefetch_auto, HIDDEN},
    {"--debug-skip", &GenOptions::debug_skip, HIDDEN}, {"--debug-drop-barrier", &GenOptions::debug_drop_barrier, HIDDEN},
};

inline bool picks(const char *pick, const std::string &v) {
    std::istringstream is(pick);
    for (std::string w; is >> w;)
        if (w == v) return true;
    return false;
}

// One scan of args (argv[1..], the .stc path last) into res.opt, from the defaults; banner: the options as the emitted source echoes
// them.  false: res.messages and res.exit_code say why, by the reference's rules (header comment).  A value option takes the next word
// whatever it looks like; the last value wins.
inline bool scan_options(const std::vector<std::string> &args, GenResult &res, std::string &banner) {
    GenOptions &o = res.opt = GenOptions();
    banner.clear();
    auto illegal = [&](int code) { res.messages += "Illegal input.\n"; res.exit_code = code; return false; };
    // With a per-axis boundary option on the line the four boundary options are echoed once, in canonical spelling (plan.hpp:
    // boundary_words), where the first of them stands: three equal per-axis values are the same command as --boundary v, and all-fixed
    // leaves no trace.  Without one, --boundary is echoed where it stands, as it always was.
    struct Echo { std::string w; bool slab, boundary; };
    std::vector<Echo> words;
    long first_boundary = -1;
    bool per_axis = false;
    auto echo = [&](const std::string &w, bool slab) { words.push_back({w, slab, false}); };
    for (size_t i = 0, stc = args.size() - 1; i < stc; i++) {
        const std::string &a = args[i];
        const Opt *r = std::find_if(std::begin(kOptions), std::end(kOptions), [&](const Opt &x) { return a == x.name; });
        if (r == std::end(kOptions)) return illegal(0);
        if (!(r->attr & NAMES)) o.tuning_given = true;
        const bool flag = r->b || (r->attr & SET1);
        if (!flag && i + 1 == stc) {
            if (a != "-o") return illegal(255);
            echo(a, false);
            continue;
        }
        const std::string v = flag ? "" : args[++i];
        if (r->b) o.*r->b = true;
        else if (flag) o.*r->i = 1;
        else if (r->i) o.*r->i = atoi(v.c_str());
        else if (r->s) o.*r->s = v;
        else if (!r->put(o, v)) return illegal(255);
        if (r->mark) o.*r->mark = true;
        if (a.compare(0, 10, "--boundary") == 0) {
            if (first_boundary < 0) first_boundary = (long)words.size();
            if (a != "--boundary") per_axis = true;
            // `--boundary fixed` is the default spelled out: it leaves no trace in the emitted source (banner and slab host alike)
            else if (v != "fixed") { words.push_back({a, true, true}); words.push_back({v, true, true}); }
            continue;
        }
        if (a == "--time-order" && o.time_order == 1) continue;       // likewise
        if (a == "--dirichlet") continue;                             // echoed once, behind every other option (below)
        if (a == "--scale" || a == "--scale-centre") continue;        // likewise, behind --dirichlet
        if (a == "--varcoef") continue;                               // likewise, behind every other option
        echo(a, !(r->attr & LOCAL));
        if (!flag) echo(v, !(r->attr & LOCAL));
    }
    for (const Opt &r : kOptions)
        if (r.pick && (!r.mark || o.*r.mark || !(o.*r.s).empty()) && !picks(r.pick, o.*r.s)) return illegal(255);
    if (o.step < 1) return illegal(255);
    if (o.time_order != 1 && o.time_order != 2) return illegal(255);
    // an explicit --dist selects the reference's kind of reuse: `Range` source planes resident, the rest carried as partial sums
    if (!o.schedule_set && o.dist != 0) o.schedule = "reuse";
    if (per_axis) {
        words.erase(std::remove_if(words.begin(), words.end(), [](const Echo &e) { return e.boundary; }), words.end());
        const int m[3] = {boundary_mode_of(o.axis_boundary(0)), boundary_mode_of(o.axis_boundary(1)), boundary_mode_of(o.axis_boundary(2))};
        long at = first_boundary;
        for (auto &w : boundary_words(o.is3d ? 3 : 2, m)) words.insert(words.begin() + at++, {w, true, true});
    }
    if (o.dirichlet) words.push_back({"--dirichlet", true, false});     // its canonical place: wherever and however often it stood, the same command
    if (o.scale) words.push_back({"--scale", true, false});
    if (o.scale_centre_set && !(o.scale && coef_rounded(o.scale_centre) == 0.0)) {       // the coefficient as the source writes it; c = 0 is the default spelled out and leaves no trace
        words.push_back({"--scale-centre", true, false});
        words.push_back({coef_text(o.scale_centre), true, false});
    }
    if (o.varcoef) words.push_back({"--varcoef", true, false});
    for (auto &e : words) { banner += (banner.empty() ? "" : " ") + e.w; if (e.slab) o.slab_args.push_back(e.w); }
    return true;
}

inline GenResult generate(const std::vector<std::string> &args /* argv[1..] */) {
    GenResult res;
    if (args.empty()) { res.messages = "Please specify the .stc file.\n"; return res; }
    if (args[0] == "--help" || args[0] == "-h") { res.messages = std::string(help_text()) + "\n"; return res; }
    std::string banner;
    if (!scan_options(args, res, banner)) return res;
    GenOptions &o = res.opt;
    const bool bare = !o.tuning_given && !o.ref_defaults;      // no geometry / emission option on the command line (the --varcoef fit rule below)
    std::vector<std::string> full_args = args;                 // the command as it is planned: with the tuner's row, if one is found

    const std::string &stcfile = args.back();
    Stencil &st = res.st;
    st.ndim = o.is3d ? 3 : 2;
    if (st.read_stc(stcfile) != 0) { res.messages += "Error opening stencil file.\n"; res.exit_code = 255; return res; }
    // No geometry / emission option on the command line: the tuner's winner for this problem class, if it has one, supplies them
    // (drstencil_amd/tuned_defaults.tsv).  The command is scanned again with the row's options in front of the .stc, so the banner's
    // `options:` line, the kernel info and the cache key are those of the explicit command line.  A row holds no naming option, so the
    // .stc as read stands.
    if (o.tuned_defaults && !o.tuning_given && !o.ref_defaults) {
        const char *mode = st.ndim == 3 ? "3d" : (o.streaming ? "2ds" : "2d");
        if (const TunedDefault *t = tuned_lookup(mode, tuned_shape_hash(st.pts), o.step, o.dtype, (o.temporal && o.step > 1) ? 1 : 0, st.N)) {
            std::vector<std::string> again(args.begin(), args.end() - 1);
            std::istringstream is(t->options);
            for (std::string w; is >> w;) again.push_back(w);
            again.insert(again.end(), {"--tuned-defaults", "0", stcfile});
            res.tuned_from = t->options;
            if (!scan_options(again, res, banner)) return res;
            full_args = again;
        }
    }
    st.fuse(o.step);
    st.choose_halo_dist(o.dist);
    if (st.partition_reuse(o.merge_forward) != REUSE_OK) { res.messages += "No data to reuse. You can try another dist.\n"; res.exit_code = 1; return res; }
    st.stream_range();

    // Round 3 default emission (no --order given): the rows order -- plane consumed by source row, partial sums pinned -- where it measured
    // faster AND is what makes the kernel fit at all: fused 3D stencils beyond 25 taps (--step 3: 256 VGPRs + scratch in the taps order,
    // 98-114 in the rows order; 1880-2080 against 430 GStencil/s at 1024^3) and one-shot 2D tiles of more than 9 taps (2d25pt_box: +6 %,
    // profiles/r03_exp_r3d.log).  Everything else keeps round 2's emission, which measured faster there (the memory-bound step-2 headline).
    // (applied after EVERY scan of the options -- the fit rule below scans again --, so that a command and the command its banner spells
    // out take the same defaults)
    auto emission_defaults = [&]() {
        if (!o.order_set && !o.ref_defaults && !o.temporal && o.schedule == "scatter" && o.stage == "reg" && std::max(o.bmy, o.cmy) == std::max(o.bmy, 1) &&
            !(o.cmx > 1 && o.cmx >= o.bmx) &&
            ((st.ndim == 3 && st.pts.size() > 25) || (st.ndim == 2 && !o.streaming && st.pts.size() > 9))) {
            o.order = "rows";
            if (o.pack < 0) o.pack = 0;       // packed pairs buy nothing with four waves per SIMD
        }
        if (o.varcoef && o.pack < 0) o.pack = 0;       // a packed pair takes ONE constant for both halves: unpacked is the default under --varcoef
    };
    emission_defaults();
    res.plan = make_plan(st, o, kernel_base_name(stcfile));
    // ---- the --varcoef fit rule.  T coefficient values per point stand in registers from their loads (in front of the plane's barrier) to
    // their FMAs: T * points-per-lane words (twice that in fp64) on top of the sweep's state.  A geometry the tuner chose for two arrays does
    // not hold them (C4: 139 VGPRs + 7 x 16), and the runtime refuses kernels that spill.  So where the command names no geometry, the
    // generator steps the planned geometry down, deterministically, until Schedule::reg_demand() plus 32 registers of addressing fits what a
    // lane can have at the workgroup's size (at most 256: no AGPR spilling): rows per lane halved down to 1, then points per row down to
    // one vector, then --by.  Each step plans the same command with the whole geometry spelled out ONCE behind the command's own words, so
    // banner, info and cache key are those of the explicit command line, and the banner's command emits this source again.  The margin of
    // 32 is not fitted to the compiler's reports.  A geometry given explicitly is taken as given
    std::string stepped_from, stepped_to;
    if (bare && o.varcoef && res.plan.error.empty()) {
        auto geometry = [](const KernelPlan &p) {
            std::vector<std::string> w = {"--bx", std::to_string(p.BX), "--by", std::to_string(p.BY), p.cyclic_x ? "--cyclic-merge-x" : "--block-merge-x", std::to_string(p.VX)};
            if (p.has_y) { w.push_back(p.cyclic_y ? "--cyclic-merge-y" : "--block-merge-y"); w.push_back(std::to_string(p.RY)); }
            if (p.has_s) { w.push_back("--sn"); w.push_back(std::to_string(p.SN)); }
            return w;
        };
        auto budget = [](const KernelPlan &p) { const int per_simd = ceil_div(ceil_div(p.NT + 64 * p.ws, 64), 4); return std::min(256, 512 / std::max(1, per_simd) / 8 * 8); };
        const std::vector<std::string> base_args = full_args;            // the command as planned first: every step starts from it
        const bool add_prefetch = res.plan.prefetch && !o.prefetch;      // the planner's default had it: the spelled-out geometry skips that default
        for (int round = 0; round < 16; round++) {
            KernelPlan &p = res.plan;
            const int demand = Schedule(p, o).reg_demand() + 32;
            if (demand <= budget(p)) break;
            KernelPlan q = p;      // the next smaller geometry
            if (p.RY > 1) q.RY = p.RY / 2;
            else if (p.VX > (p.fp32 ? 4 : 2) && p.VX % 2 == 0) q.VX = p.VX / 2;
            else if (p.BY > 1) q.BY = p.BY / 2;
            else break;
            if (stepped_from.empty()) stepped_from = joined(geometry(p)) + " (" + std::to_string(demand) + " registers per lane of " + std::to_string(budget(p)) + ")";
            // (the command itself names no geometry: such words in it are the tuner's row's, and give way to the geometry spelled out here)
            std::vector<std::string> again;
            for (size_t i = 0; i + 1 < base_args.size(); i++) {
                static const char *const geo[] = {"--bx", "--by", "--sn", "--block-merge-x", "--cyclic-merge-x", "--block-merge-y", "--cyclic-merge-y"};
                if (std::find_if(std::begin(geo), std::end(geo), [&](const char *g) { return base_args[i] == g; }) != std::end(geo)) { i++; continue; }
                again.push_back(base_args[i]);
            }
            for (auto &w : geometry(q)) again.push_back(w);
            if (add_prefetch) again.push_back("--prefetch");
            if (std::find(again.begin(), again.end(), "--tuned-defaults") == again.end()) again.insert(again.end(), {"--tuned-defaults", "0"});
            again.push_back(stcfile);
            full_args = again;
            if (!scan_options(again, res, banner)) return res;
            emission_defaults();
            res.plan = make_plan(st, o, kernel_base_name(stcfile));
            if (!res.plan.error.empty()) break;
            stepped_to = joined(geometry(res.plan));
        }
    }
    if (!res.plan.error.empty()) { res.messages += "Invalid configuration!\n"; res.exit_code = 255; res.error = res.plan.error; return res; }
    if (!res.plan.note.empty()) res.messages += "drstencil: note: " + res.plan.note + "\n";
    if (o.gpus < 1 || o.gpus > 64) { res.messages += "Illegal input.\n"; res.exit_code = 255; return res; }
    if (o.gpus > 1 || o.pair_launch) {
        // The slab runtime's views are windows of TWO arrays with every axis fixed, and the pair kernel exists only to serve it: an option
        // with no slab form refuses both.  One row per option -- {it is on, its name, why not with --gpus N > 1, what the slab runtime
        // lacks for --pair-launch 1} --, the first match wins.  Ring fill: periodic z (y in 2D) across ranks would need a rank 0 <->
        // rank N-1 exchange, and a view's ring holds ghost planes of its neighbours, which no view may refill.  Time order 2: ghost planes
        // are recomputed redundantly under every = 2 and would need valid old values too.  Residual: a rank's maximum would still have to
        // be reduced over the ranks
        const KernelPlan &p = res.plan;
        struct Refusal { bool on; std::string option; const char *gpus, *pair; };
        const Refusal rows[] = {
            {p.fills_ring(), p.periodic ? "--boundary periodic" : joined(boundary_words(st.ndim, p.bmode, false)),
             p.periodic ? "the slab runtime has no periodic exchange" : "the slab runtime keeps every axis fixed: a slab view has no ring fill",
             p.periodic ? "has no periodic exchange" : "keeps every axis fixed"},
            {p.second_order, "--time-order 2", "the slab runtime keeps no old values in its ghost planes", "has no second-order form"},
            {p.source, "--source", "the slab runtime passes no view of a source array", "has no source term"},
            {p.residual, "--residual", "the slab runtime passes no residual array and reduces nothing over the ranks", "has no residual"},
            {p.dirichlet, "--dirichlet", "the slab runtime passes no view of an array of held cells", "has no held cells"},
            {p.varcoef, "--varcoef", "the slab runtime passes no views of the coefficient grids", "has no coefficient arrays"},
            {p.scale, "--scale", "the slab runtime passes no view of an array of factors", "has no per-cell factor"},
        };
        for (const Refusal &r : rows) {
            if (!r.on) continue;
            res.messages += "Invalid configuration!\n"; res.exit_code = 255;
            res.error = r.option + " cannot be combined with " + (o.gpus > 1 ? std::string("--gpus N > 1 (") + r.gpus : std::string("--pair-launch 1 (the pair kernel serves the slab runtime, which ") + r.pair) + ")";
            return res;
        }
    }
    const Schedule sched(res.plan, o);
    if (!sched.config_error().empty()) { res.messages += "Invalid configuration!\n"; res.exit_code = 255; res.error = sched.config_error(); return res; }
    if (sched.lds_bytes() > 160 * 1024) {   // gfx950: 160 KiB of LDS per workgroup
        res.messages += "Invalid configuration!\n"; res.exit_code = 255; res.error = "tile needs more than 160 KiB of LDS"; return res;
    }
    res.source = HipEmitter(sched).source(stcfile, banner);
    if (res.plan.periodic) {
        const int H = st.halo;
        std::string per = st.ndim == 3 ? std::to_string(st.L - 2 * H) + " x " : "";
        per += std::to_string(st.M - 2 * H) + " x " + std::to_string(st.N - 2 * H);
        res.notes += "drstencil: note: periodic boundaries: period " + per + ", ring of width " + std::to_string(H) + " holds ghost copies\n";
    } else if (res.plan.fills_ring()) {
        std::string axes;
        for (int a = st.ndim == 3 ? 0 : 1; a < 3; a++) axes += std::string(axes.empty() ? "" : ", ") + "zyx"[a] + " " + boundary_mode_name(res.plan.bmode[a]);
        res.notes += "drstencil: note: boundaries per axis: " + axes + "; the ring of width " + std::to_string(st.halo) +
                     " on the non-fixed axes holds ghost copies (periodic images / zero-flux mirror images of the interior)\n";
    }
    if (o.step > 1) {
        // a fused launch (and a temporal pipeline) applies S^n to the mirrored extension: n mirrored one-step updates only when the one-step
        // stencil is its own mirror image along every reflecting axis
        std::string odd;
        for (int a = 0; a < 3; a++) {
            if (res.plan.bmode[a] != REFLECT) continue;
            bool sym = true;
            for (auto &e : st.base.v) {
                Pt m = e.first;
                (a == 0 ? m.k : a == 1 ? m.j : m.i) = -e.first.at(a);
                sym = sym && st.base.has(m) && st.base.get(m) == e.second;
            }
            if (!sym) odd += std::string(odd.empty() ? "" : ", ") + "zyx"[a];
        }
        if (!odd.empty())
            res.notes += "drstencil: note: the one-step stencil is not symmetric along the reflecting axis " + odd + ": a --step " + std::to_string(o.step) +
                         " launch applies the fused stencil to the mirrored extension, which differs from " + std::to_string(o.step) + " mirrored one-step updates near those walls\n";
    }
    if (res.plan.second_order)
        res.notes += "drstencil: note: second-order time stepping: a launch computes out = S(in) - out_old on the interior (the output array's interior is input)\n";
    if (res.plan.source)
        res.notes += std::string("drstencil: note: source term: a launch takes a third array and computes out = ") +
                     (res.plan.second_order ? "(S(in) - out_old) + src" : "S(in) + src") + " on the interior (src is read only, in its interior)\n";
    if (res.plan.residual)
        res.notes += "drstencil: note: residual: a launch takes one more array of " + std::to_string(sched.residual_elems()) + " elements and writes r = max |out - in| over the interior to its first element (NaN if any term is NaN)\n";
    if (res.plan.dirichlet)
        res.notes += "drstencil: note: held cells: a launch takes one more array fix and stores fix[p] wherever it is not NaN, else the computed value (fix is read only, in its interior)\n";
    if (res.plan.scale)
        res.notes += std::string("drstencil: note: per-cell factor: a launch takes one more array w and computes ") +
                     (res.plan.centre_term() ? "(" + res.plan.scale_centre + ") * in + w * S(in)" : std::string("w * S(in)")) + " on the interior, in front of the other options' operations (w is read only, in its interior)\n";
    if (res.plan.varcoef)
        res.notes += "drstencil: note: per-tap coefficients: a launch takes one more array coef of " + std::to_string(res.plan.taps.size()) +
                     " grids, tap t's in grid t (gold order, \"coef_taps\" in the kernel info), and computes sum_t coef[t][p] * in[p + d_t] as the FMA chain; the .stc constants are not used (coef is read only, in its interior)\n";
    if (!stepped_to.empty())
        res.notes += "drstencil: note: --varcoef: no geometry option given and " + stepped_from + " does not hold the " + std::to_string(res.plan.taps.size()) +
                     " coefficient values per point; stepped down to " + stepped_to + "\n";
    if (!res.tuned_from.empty())
        res.notes += "drstencil: note: no geometry option given: the tuner's configuration for this stencil, step, dtype and grid size is used (" +
                     res.tuned_from + "); --tuned-defaults 0 keeps the generic defaults\n";
    res.out_name = o.out_name;
    res.emitted = true;
    return res;
}

inline bool write_text(const std::string &path, const std::string &text) {
    std::ofstream f(path, std::ios::out | std::ios::trunc);
    if (!f) return false;
    f << text;
    return (bool)f;
}

}  // namespace drs
