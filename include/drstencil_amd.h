/*
 * drstencil_amd.h -- C ABI of libdrstencil_amd.so (MI355X-native DRStencil generator + runtime).
 *
 * The reference (simple86/DRStencil) has NO library/FFI surface: its boundary is the
 * `drstencil` command line, the .stc file format and the emitted program.
 * Each entry point below names the reference interface it stands for; INTEGRATION.md shows
 * how a maintainer binds it.  Plain C types only; device buffers are raw device pointers
 * (e.g. torch.Tensor.data_ptr()), streams are hipStream_t passed as void*.
 */
#ifndef DRSTENCIL_AMD_H
#define DRSTENCIL_AMD_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct drs_spec drs_spec;     /* parsed + fused stencil, reuse analysis done */
typedef struct drs_kernel drs_kernel; /* generated, compiled (hipcc, gfx950) and loaded kernel */

/* ---- generator: the `drstencil [options] file.stc` command as a function.
 * Replaces main() of main.cpp:10-280 (option scan 118-230, pipeline 237-278).
 * argv excludes the program name.  Returns the process exit code the command would have
 * (0, 1 "No data to reuse", 255 "Illegal input."/"Invalid configuration!"/"Error opening
 * stencil file.").  *source (emitted HIP text, NULL if nothing was emitted) and *messages
 * (the command's stdout text, followed by what it prints on stderr: remarks such as "the tuner's configuration ... is used") are malloc'ed; release with drs_free.  No file is written. */
int drs_generate(int argc, const char *const *argv, char **source, char **messages);
void drs_free(void *p);

/* ---- stencil IR: DRStencil / DRStencil_2d (drstencil.hpp:15-49, drstencil_2d.hpp).
 * drs_spec_open = get_stencil (52-78) + fusing (262-282) + dataReuse (306-311).
 * *status: 0 ok, 1 cannot open the file, 2 "No data to reuse" (spec still returned). */
drs_spec *drs_spec_open(const char *stc_path, int ndim, int step, int dist, int merge_forward, int *status);
void drs_spec_close(drs_spec *s);
int drs_spec_halo(const drs_spec *s);        /* get_order()    drstencil.hpp:34 */
int drs_spec_dist(const drs_spec *s);        /* get_distance() drstencil.hpp:35 */
int drs_spec_range(const drs_spec *s);       /* high_k - low_k + 1, codegen.hpp:89 */
int drs_spec_npoints(const drs_spec *s);     /* fused stencil size */
int drs_spec_iterations(const drs_spec *s);  /* get_problem_size, drstencil.hpp:80-86 */
int drs_spec_launches(const drs_spec *s);    /* kernel launches of the timed loop, codegen.hpp:581-584 */
void drs_spec_dims(const drs_spec *s, int *L, int *M, int *N);
/* point idx in gold (lexicographic) order; coef_text = the 6-significant-digit literal
 * the emitted source carries (drstencil.hpp:192), at least 32 bytes */
int drs_spec_point(const drs_spec *s, int idx, int *k, int *j, int *i, double *coef, char *coef_text);
/* sizes of forward_k, forward_j, forward_i, backward (partition, drstencil.hpp:198-259) */
void drs_spec_partition(const drs_spec *s, int sizes[4]);

/* ---- runtime: what the emitted program's main() does (host_code_gen, codegen.hpp:547-635),
 * callable on caller-owned device buffers.
 * drs_kernel_build: generate (same argv as drs_generate), compile with hipcc for gfx950 into
 * cache_dir (NULL: <package>/_kcache) unless already cached, and load.  NULL on failure with
 * *log (malloc'ed, may be NULL) holding the generator messages / compiler output. */
drs_kernel *drs_kernel_build(int argc, const char *const *argv, const char *cache_dir, char **log);
void drs_kernel_close(drs_kernel *k);                /* frees the handle; the plugin stays mapped (safe at process exit) */
/* drs_kernel_close + the plugin is unloaded (hipDeviceSynchronize, then dlclose: its code object leaves the HIP runtime).
 * For long sweeps that load thousands of kernels (the tuner: benchmarks/3d7pt_star/tuning.py:102-142 starts one process
 * per configuration instead).  Not to be called while one of its launches may still be running on another device. */
int drs_kernel_unload(drs_kernel *k);
/* JSON: dims, dtype, halo, step, grid, lds ... and which arithmetic the kernel computes:
 *   "arithmetic": "gold-order"    the reference's fused sum (drstencil.hpp:182-196, 262-282) as one FMA chain -- bit-identical
 *                                  to gold_<name> for any iteration count ("tolerance_horizon_iterations": -1);
 *                 "reassociated"  on-chip time steps (--temporal 1 / force): equal to it up to rounding; the generator emits
 *                                  such a kernel only where its drift estimate ("drift_estimate", relative, for the spec's
 *                                  iterations) stays within 1e-6 (fp32) / 1e-12 (fp64), "tolerance_horizon_iterations" is the
 *                                  largest iteration count for which it does, and "temporal_forced": 1 marks --temporal force.
 *   "out_skew_bytes", "placement_period_bytes": where the output array should sit relative to the input array, modulo the period
 *                                  (64 MiB): see drs_kernel_pair_layout below.
 *   "boundary": "periodic", "period": [P...]   only for kernels generated with --boundary periodic (see drs_kernel_wrap).
 *   "boundary": "reflect" | "mixed", "boundaries": [modes, outermost axis first]   kernels with a reflecting axis or with axes of
 *                                  different modes (--boundary reflect, --boundary-z / -y / -x): "fixed" | "periodic" | "reflect" per
 *                                  axis, three entries in 3D, two in 2D.  Neither key: every axis is fixed.
 *   "time_order": 2                only for kernels generated with --time-order 2 (see drs_kernel_launch).
 *   "source": 1                    only for kernels generated with --source (see drs_kernel_launch_src).
 *   "dirichlet": 1                 only for kernels generated with --dirichlet (see drs_kernel_launch_fix).
 *   "scale": 1, "scale_centre": C  only for kernels generated with --scale (see drs_kernel_launch_ops): C is 0 without a centre term.
 *   "varcoef": 1, "coef_taps": [[k,j,i],...]   only for kernels generated with --varcoef (see drs_kernel_launch_ops): tap t of coef, gold order.
 *   "residual": "max", "residual_elems": N   only for kernels generated with --residual max (see drs_kernel_launch_res): N = 1 + "grid". */
const char *drs_kernel_info(const drs_kernel *k);
const char *drs_kernel_path(const drs_kernel *k);   /* the loaded shared object */
/* JSON: vgprs, agprs, sgprs, scratch_bytes_per_lane, sgpr_spill, vgpr_spill, occupancy_waves_per_simd, lds_bytes of
 * dr_<name> (with --pair-launch: the maximum over dr_<name> and dr2_<name>) as reported by hipcc -- what the reference reads
 * from `ncu --set full`, getGpuMetrics.py:9 -- plus "verified": 1 when every field was found in the compiler's report.
 * drs_kernel_build refuses (NULL + log): a kernel that spills to scratch or spills scalar registers (sgpr_spill > 0;
 * DRS_ALLOW_SCRATCH=1 overrides either), a kernel whose
 * report could not be read (DRS_ALLOW_UNVERIFIED=1), a cache miss once this process has launched a kernel or when
 * DRS_NO_COMPILE=1 (hipcc is a child process: build first, launch afterwards), and --debug-drop-barrier kernels
 * (wrong results by design) without DRS_EXPERIMENTS=1. */
const char *drs_kernel_resources(const drs_kernel *k);
/* Where to put the two arrays.  The reference's host code makes two cudaMalloc calls (codegen.hpp:556-566); on MI355X the
 * launch time of a z-streaming kernel depends on (out - in) mod 64 MiB -- up to 14 % for the 1024^3 step-2 kernel
 * (profiles/r03_probe_skew4.log) -- so the emitted program and bench.py carve both arrays out of ONE allocation:
 * in = arena, out = arena + *out_offset (a multiple of the 64 MiB period that clears the array + the kernel's "out_skew_bytes"),
 * arena of *arena_bytes.  Advice only: every entry point accepts any two device pointers, results never depend on them. */
int drs_kernel_pair_layout(const drs_kernel *k, size_t *arena_bytes, size_t *out_offset);
/* one launch of dr_<name><<<grid, block, 0, stream>>>(in, out): codegen.hpp:577,582-583.
 * Kernels with a non-fixed axis (--boundary periodic | reflect, --boundary-z / -y / -x) first run wrap_<name> on d_in
 * (drs_kernel_wrap), so d_in's RING IS OVERWRITTEN ON ITS NON-FIXED AXES although the parameter is const; the result depends only on d_in's interior, and d_out's ring is not touched.  The same holds for
 * drs_kernel_launch_gold, drs_kernel_run and drs_kernel_run_timed, whose launches go through the same entry points.
 * --time-order 2 kernels compute d_out = S(d_in) - d_out on the interior: d_out's INTERIOR IS INPUT (each cell's old value reaches
 * only that cell; d_out's ring is neither read nor written).  The ping-pong loop of drs_kernel_run is then the leapfrog scheme
 * u(t+1) = S(u(t)) - u(t-1) with d_a = u(t), d_b = u(t-1); the same holds for drs_kernel_launch_gold.  Such kernels need --step 1;
 * --temporal, --gpus N > 1, --pair-launch 1 and the drs_slab_* runtime refuse them. */
int drs_kernel_launch(drs_kernel *k, const void *d_in, void *d_out, void *stream);
/* one launch of dr2_<name>: the same sweep over TWO (in, out) pairs (kernels generated with --pair-launch 1; -2 otherwise).
 * No reference counterpart: the two boundary views of a slab-decomposed run (drstencil_amd/multigpu.py) in one launch. */
int drs_kernel_launch_pair(drs_kernel *k, const void *d_in0, void *d_out0, const void *d_in1, void *d_out1, void *stream);
/* one launch of gold_<name> (the reference's verification kernel, codegen.hpp:611-612) */
int drs_kernel_launch_gold(drs_kernel *k, const void *d_in, void *d_out, void *stream);
/* --boundary periodic (no reference counterpart: the reference's ring is a fixed Dirichlet boundary).  The grid's interior is a
 * periodic domain of period P_d = dim_d - 2 * Halo in every dimension (Halo = step * order, so P depends on --step), and its ring
 * of width Halo holds ghost copies: the ghost at coordinate x takes the value at w(x) = x + P (x < Halo), x - P (x >= dim - Halo),
 * x otherwise, each coordinate wrapped on its own (edges and corners included).  One launch of wrap_<name> on d, asynchronous on
 * `stream`: fills d's ring from d's interior (the interior is not written).
 * --boundary reflect: zero-flux walls on the faces between ring and interior: the ghost takes m(x) = 2 Halo - 1 - x (x < Halo),
 * 2 (dim - Halo) - 1 - x (x >= dim - Halo) -- the ghost at distance d outside a face is the interior cell at distance d - 1 inside
 * (numpy's pad mode "symmetric").  --boundary-z / -y / -x choose the mode per axis; a fixed axis maps every coordinate to itself
 * and its ring is never written.  A ring cell is filled iff one of its coordinates lies in the ring of a non-fixed axis, from the
 * cell with every coordinate mapped on its own (which may lie in the ring of a fixed axis).  A fused --step n launch applies S^n
 * to the mirrored extension: n mirrored one-step updates only for a one-step stencil symmetric along every reflecting axis.
 * -2 when every axis of the kernel is fixed.  A non-fixed axis needs a dimension >= 3 * Halo; --gpus N > 1, --pair-launch 1 and
 * the drs_slab_* runtime refuse every non-fixed axis. */
int drs_kernel_wrap(drs_kernel *k, void *d, void *stream);
/* the timed ping-pong loop: for (t = 0; t < iterations; t += 2*step) { k(A,B); k(B,A); }
 * (codegen.hpp:581-584).  gold != 0 runs gold_<name> instead.  Returns the number of
 * launches, -1 on a HIP error, or -3 when `iterations` exceeds the tolerance horizon of a reassociated (temporal) kernel
 * that was not built with --temporal force: build the fused kernel for such a run.  Asynchronous on `stream`. */
int drs_kernel_run(drs_kernel *k, void *d_a, void *d_b, int iterations, int gold, void *stream);
/* `warmup` untimed launches (A,B) (codegen.hpp:575-578), then the loop above bracketed by
 * HIP events recorded on `stream`; blocks until done; *ms = elapsed milliseconds.  With a --time-order 2 kernel the warm-up
 * launches ADVANCE THE STATE (each reads and rewrites d_b's interior): restore both arrays afterwards if the values matter. */
int drs_kernel_run_timed(drs_kernel *k, void *d_a, void *d_b, int iterations, int warmup, void *stream, float *ms);

/* ---- --source kernels: a third, read-only operand ---------------------------------------------------------------------------------
 * A kernel generated with --source is dr_<name>(in, out, src): d_out = S(d_in) + d_src on the interior, and with --time-order 2
 * d_out = (S(d_in) - d_out) + d_src, each operation rounded on its own.  d_src has the grid's shape and dtype; only its INTERIOR is read,
 * each value reaching only its own cell, and it is never written.  It must not overlap d_out (it may be d_in); it follows the
 * alignment rule of the other two arrays.  Its plugin exports the three-pointer launch entry points INSTEAD of the two-pointer ones:
 * drs_kernel_launch, _launch_gold, _run and _run_timed return -2 on such a kernel, and the four below return -2 on a kernel
 * generated without --source and on a null d_src.  The loops pass the same d_src to every launch: k(A,B,F); k(B,A,F).  Everything said
 * of the two-pointer forms (ring fill on d_in first, warm-up of an order-2 kernel advancing the state, -3 beyond a tolerance horizon)
 * holds unchanged; --step n > 1, --temporal, --gpus N > 1, --pair-launch 1 and the drs_slab_* runtime refuse --source. */
int drs_kernel_launch_src(drs_kernel *k, const void *d_in, void *d_out, const void *d_src, void *stream);
int drs_kernel_launch_gold_src(drs_kernel *k, const void *d_in, void *d_out, const void *d_src, void *stream);
int drs_kernel_run_src(drs_kernel *k, void *d_a, void *d_b, const void *d_src, int iterations, int gold, void *stream);
int drs_kernel_run_timed_src(drs_kernel *k, void *d_a, void *d_b, const void *d_src, int iterations, int warmup, void *stream, float *ms);

/* ---- --residual max kernels: the convergence residual of every launch, fused into the sweep ----------------------------------------------
 * No reference counterpart.  A kernel generated with --residual max is dr_<name>(in, out[, src], res): beside the sweep it writes
 *     d_res[0] = max over the interior of |d_out - d_in|
 * in the grid's dtype, d_out being the value the launch stores (after - out_old and + src where those options are on), the difference one
 * rounded subtraction, |.| clearing the sign, and the maximum PROPAGATING NaN (NaN if any term is NaN, else the largest term, +0.0 for an
 * all-zero difference): bit for bit numpy's max(abs(out[I] - in[I])).  With a fused --step n it is max |S^n(in) - in|.  The stored arrays
 * are those of the same command without the option.
 * d_res holds drs_kernel_residual_elems(k) = 1 + grid elements of the grid's dtype (0 for a kernel without the option; "residual_elems" of
 * the kernel info): [0] the result, then one partial per launched workgroup.  Every launch WRITES ALL OF THEM and reads only what it has
 * written itself: the caller initialises nothing and nothing carries over between launches.  d_res is element aligned and must not overlap the
 * other arrays.  A launch also reads d_in at every interior cell (new only for stencils without a centre tap); it touches nothing outside
 * the arrays.  The launch enqueues two kernels on `stream`: the sweep, then res_<name>, one workgroup that folds the partials.
 * The plugin exports drs_plugin_launch_res INSTEAD of the sweep's launch entry point: drs_kernel_launch, _launch_src, _run, _run_src,
 * _run_timed and _run_timed_src return -2 on such a kernel, and the entry points below return -2 on a kernel generated without
 * --residual, on a null d_res, and when d_src does not go with the kernel (null on a --source kernel, non-null on one without).
 * gold_<name> computes no residual and keeps its entry points (drs_kernel_launch_gold / _launch_gold_src): a reference takes the
 * residual from gold's arrays on the host.  -1 is a HIP error.  --temporal, --gpus N > 1, --pair-launch 1 and the drs_slab_* runtime
 * refuse --residual. */
long drs_kernel_residual_elems(const drs_kernel *k);
/* one launch (in -> out) and its residual into d_res[0]; asynchronous on `stream` */
int drs_kernel_launch_res(drs_kernel *k, const void *d_in, void *d_out, const void *d_src, void *d_res, void *stream);
/* the reference's loop, for (t = 0; t < iterations; t += 2*step) { k(A,B); k(B,A); }: the number of launches; d_res[0] then holds the LAST
 * launch's residual.  Asynchronous on `stream`. */
int drs_kernel_run_res(drs_kernel *k, void *d_a, void *d_b, const void *d_src, void *d_res, int iterations, void *stream);
/* drs_kernel_run_timed with the residual array: `warmup` launches (A,B), then the loop above between two events; blocks until done */
int drs_kernel_run_timed_res(drs_kernel *k, void *d_a, void *d_b, const void *d_src, void *d_res, int iterations, int warmup, void *stream, float *ms);
/* d_res[0] of a --residual kernel copied to the host as a double (exact for either dtype); the copy synchronises with the device */
int drs_kernel_residual(const drs_kernel *k, const void *d_res, double *r);
/* Run to tolerance.  Repeats: enqueue `check_every_pairs` (>= 1) ping-pong pairs k(A,B); k(B,A) -- fewer when `max_launches`, rounded down
 * to an even number, would be passed --, synchronise `stream`, copy d_res[0] (the last launch's residual r) to the host, decide:
 *     0   r <= tol
 *     1   max_launches reached (also when it allows no pair: *launches = 0, *residual = NaN)
 *    -4   r is NaN or inf: a diverged or overflowed run is reported instead of iterated on
 * (-2 and -1 as above).  *launches = launches made, *residual = the last r read (either may be NULL).  The answer is always in d_a. */
int drs_kernel_solve(drs_kernel *k, void *d_a, void *d_b, const void *d_src, void *d_res, double tol, int max_launches, int check_every_pairs, void *stream,
                     int *launches, double *residual);

/* ---- --dirichlet kernels: held cells inside the domain ---------------------------------------------------------------------------------
 * No reference counterpart.  A kernel generated with --dirichlet is dr_<name>(in, out[, src][, res], fix).  d_fix has the grid's shape
 * and dtype; at every interior point p the launch stores d_out[p] = (d_fix[p] != d_fix[p]) ? v : d_fix[p], where v is the value the same
 * command without the option would store (S(in), then - out_old with --time-order 2, then + src with --source).  A cell whose fix is
 * NaN -- either sign, any payload, signalling ones included -- is FREE; every other cell is HELD and receives d_fix[p] bit for bit
 * (+-0.0, subnormals and +-inf are legal held values).  The choice is a select, never arithmetic: a held cell whose v is NaN or inf still
 * receives d_fix[p], and a free cell receives exactly v.  S(in) reads d_in as it is -- at a held neighbour q it uses d_in[q], not
 * d_fix[q] -- so after one launch the output holds the held values and after a ping-pong pair both arrays do; a caller who wants the
 * first launch consistent writes fix's held values into A first (and into B with --time-order 2).  With --residual max, r is max |out - in|
 * over the whole interior of the stored arrays, held cells included (they contribute +0.0 once d_in holds them).  Only the INTERIOR of
 * d_fix is read, each value reaching only its own cell; it is never written, must not overlap d_out, and follows the alignment rule of
 * the other arrays.  Ring fills touch d_in only.
 * Such a plugin exports drs_plugin_launch_fix / drs_plugin_launch_gold_fix INSTEAD of every other launch entry point: drs_kernel_launch,
 * _launch_gold, _run, _run_timed and the _src / _res families and drs_kernel_solve return -2 on it, and the five below return -2 on a
 * kernel generated without --dirichlet, on a null d_fix, and when d_src / d_res do not go with the kernel: d_src is non-null exactly
 * on a --source kernel, d_res (drs_kernel_residual_elems(k) elements) exactly on a --residual max kernel.  -1 is a HIP error.
 * --step n > 1, --temporal, --gpus N > 1, --pair-launch 1 and the drs_slab_* runtime refuse --dirichlet. */
/* drs_kernel_launch / _launch_src / _launch_res with held cells: one launch (in -> out), asynchronous on `stream` */
int drs_kernel_launch_fix(drs_kernel *k, const void *d_in, void *d_out, const void *d_src, void *d_res, const void *d_fix, void *stream);
/* drs_kernel_launch_gold / _launch_gold_src with held cells: gold_<name>(in, out[, src], fix), which computes no residual */
int drs_kernel_launch_gold_fix(drs_kernel *k, const void *d_in, void *d_out, const void *d_src, const void *d_fix, void *stream);
/* drs_kernel_run / _run_src / _run_res with held cells: the ping-pong loop k(A,B,..,F); k(B,A,..,F) with the same arrays in every launch;
 * gold != 0 runs gold_<name> (d_res is then left alone).  Returns the launches made. */
int drs_kernel_run_fix(drs_kernel *k, void *d_a, void *d_b, const void *d_src, void *d_res, const void *d_fix, int iterations, int gold, void *stream);
/* drs_kernel_run_timed / _run_timed_src / _run_timed_res with held cells: `warmup` launches (A,B), then the loop between two events */
int drs_kernel_run_timed_fix(drs_kernel *k, void *d_a, void *d_b, const void *d_src, void *d_res, const void *d_fix, int iterations, int warmup, void *stream, float *ms);
/* drs_kernel_solve with held cells: the same loop and the same answers (0, 1, -4; -2 also on a kernel without --residual max) */
int drs_kernel_solve_fix(drs_kernel *k, void *d_a, void *d_b, const void *d_src, void *d_res, const void *d_fix, double tol, int max_launches, int check_every_pairs,
                         void *stream, int *launches, double *residual);

/* ---- the operand block: every array a launch takes beside in and out ------------------------------------------------------------------
 * No reference counterpart.  One family of entry points for EVERY kernel, old kinds included, instead of one suffixed family per option.
 * The caller sets size = sizeof(drs_operands) and each pointer the kernel takes, NULL for the others:
 *   src    --source         read only, the grid's shape and dtype
 *   res    --residual max   drs_kernel_residual_elems(k) elements, written whole by every launch
 *   fix    --dirichlet      read only, the grid's shape and dtype
 *   scale  --scale          read only, the grid's shape and dtype
 *   coef   --varcoef        read only, T grids of the grid's shape and dtype, tap t's first (see below)
 * -2 (the "wrong kind" code of every family): size is not sizeof(drs_operands), a pointer the kernel needs is NULL, or a pointer the kernel
 * does not take is non-NULL.  The gold kernel computes no residual: the gold forms leave res alone, and accept one only on a --residual
 * max kernel.  -1 is a HIP error, -3 as drs_kernel_run.
 * --scale: a kernel generated with --scale is dr_<name>(in, out[, src][, res][, fix], w).  At every interior point p it computes
 *   v = S(in)[p]  (the unchanged FMA chain);  v = w[p] * v;  with --scale-centre c != 0: t = C * in[p]; v = t + v;
 * then - out_old[p] (--time-order 2), + src[p] (--source), the --dirichlet select, the residual update and the store, as without the
 * option.  Every operation is rounded once, nothing is contracted.  C is c as a coefficient is written (six digits, cast to the dtype;
 * "scale_centre" in drs_kernel_info).  Only the INTERIOR of w is read, each value reaching only its own cell; w is never written, must not
 * overlap d_out and follows the alignment rule of the other arrays.  Ring fills touch d_in only.  With w = 1 everywhere and no centre
 * term the stored bits are those of the same command without the option.
 * Such a plugin exports drs_plugin_launch_ops / drs_plugin_launch_gold_ops INSTEAD of every other launch entry point: every entry point
 * above (the plain, _src, _res and _fix families and drs_kernel_solve) returns -2 on it; it runs through the five below only.
 * --step n > 1, --temporal, --gpus N > 1, --pair-launch 1 and the drs_slab_* runtime refuse --scale.
 * --varcoef: a kernel generated with --varcoef is dr_<name>(in, out[, src][, res][, fix][, w], coef).  coef has the grid's dtype and shape
 * (T, L, M, N) -- (T, M, N) in 2D --, T = "taps"; grid t starts at element t * L * M * N (64-bit offsets) and holds the coefficient of tap t
 * of the gold sum, the taps being listed by "coef_taps" / drs_kernel_coef_taps.  At every interior point p
 *   v = a_0[p] * in[p + d_0];  v = fma(a_t[p], in[p + d_t], v), t = 1 .. T-1
 * -- the unchanged chain with the array value in the constant's place; the .stc constants give the shape and the order only -- and then
 * the operations above in their order.  Only the INTERIOR of each grid is read, each value reaching only its own cell and its own tap;
 * coef is never written, must not overlap d_out and follows the alignment rule of the other arrays.  With a_t = the constant as it is
 * written, everywhere, the stored bits are those of the same command without the option.  Such a kernel runs through the five entry
 * points below only: every suffixed family and the plain entry points return -2 on it.  --step n > 1, --temporal, --gpus N > 1,
 * --pair-launch 1, --coef, --pack 1 and the drs_slab_* runtime refuse --varcoef.
 * The block grew by its trailing field `coef` with --varcoef, and size is still checked strictly: a caller compiled against the older,
 * shorter block gets -2 from every _ops entry point -- never a read past its block -- and has to be recompiled. */
typedef struct { size_t size; const void *src; void *res; const void *fix; const void *scale; const void *coef; } drs_operands;
/* "[[k,j,i],...]": the taps of a --varcoef kernel in the order of coef's grids (k = 0 in 2D); NULL for any other kernel.  Owned by k. */
const char *drs_kernel_coef_taps(const drs_kernel *k);
/* one launch (in -> out), asynchronous on `stream` */
int drs_kernel_launch_ops(drs_kernel *k, const void *d_in, void *d_out, const drs_operands *ops, void *stream);
/* gold_<name> with the same operands */
int drs_kernel_launch_gold_ops(drs_kernel *k, const void *d_in, void *d_out, const drs_operands *ops, void *stream);
/* the ping-pong loop k(A,B,ops); k(B,A,ops); gold != 0 runs gold_<name>.  Returns the launches made. */
int drs_kernel_run_ops(drs_kernel *k, void *d_a, void *d_b, const drs_operands *ops, int iterations, int gold, void *stream);
/* `warmup` launches (A,B), then the loop between two events */
int drs_kernel_run_timed_ops(drs_kernel *k, void *d_a, void *d_b, const drs_operands *ops, int iterations, int warmup, void *stream, float *ms);
/* drs_kernel_solve through the operand block (0, 1, -4; -2 also on a kernel without --residual max) */
int drs_kernel_solve_ops(drs_kernel *k, void *d_a, void *d_b, const drs_operands *ops, double tol, int max_launches, int check_every_pairs, void *stream,
                         int *launches, double *residual);

/* ---- N > 1: one rank of a slab-decomposed run (z slabs in 3D, y slabs in 2D), one process per GPU -----------------------------
 * No reference counterpart: the reference is single-GPU (no cudaSetDevice / streams / NCCL anywhere; SURVEY.md section 5 sketches
 * this layer as `ncclGroupStart; ncclSend/ncclRecv x <= 4; ncclGroupEnd` on a comm stream).  What these entry points must
 * reproduce is the SINGLE-DOMAIN run of drs_kernel_run on the whole grid, bit for bit; drstencil_amd/multigpu.py (SlabPlan /
 * SlabRun, the torch.distributed path) is the reference implementation they are tested against.
 *   rank 0:      drs_slab_unique_id(id)                  -> hand the 128 bytes to every rank (MPI_Bcast, a file, a socket ...)
 *   every rank:  s = drs_slab_open(argc, argv, ..., world, rank, every, 0, cache, &log)   plan + kernels, BEFORE any GPU call
 *                                                          (it may start hipcc); argv = generator options + the whole grid's .stc
 *                hipSetDevice(local_rank); drs_slab_connect(s, id, stream)    ncclCommInitRank, side stream, events
 *                drs_slab_plan(s, p): this rank holds global planes [p[0], p[1]) = Lloc planes INCLUDING G ghost planes per
 *                                     interior face, owns [p[2], p[3]); A and B are caller-owned device buffers of that size
 *                n = drs_slab_run(s, d_a, d_b, iterations)                    the reference's loop (codegen.hpp:581-584) on the slab
 *                drs_slab_sync(s); drs_slab_close(s)
 * every = 1: each launch exchanges its output's H = step * order boundary planes with the <= 2 neighbours; every = 2: ghost
 * planes 2H wide, one exchange per ping-pong pair.  A pair is captured once into a HIP graph per (A, B) and replayed
 * (DRS_SLAB_GRAPH=0: eager); drs_slab_info tells ("graph": 1 captured, -1 refused -> eager).  rehearse_world > 0 plays rank
 * `rank` of `rehearse_world` on ONE GPU with itself as both neighbours (communicator of size 1): tests and one-GPU rehearsals.
 * drs_slab_run answers -1 on an error (drs_slab_error) and -3, like drs_kernel_run, when the slab was opened with `--temporal 1`
 * options (on-chip stages, reassociated arithmetic) and `iterations` exceeds the kernels' tolerance horizon. */
typedef struct drs_slab drs_slab;
#define DRS_SLAB_ID_BYTES 128
int drs_slab_unique_id(void *id128);
drs_slab *drs_slab_open(int argc, const char *const *argv, int alone_argc, const char *const *alone_argv, int world, int rank, int every,
                        int rehearse_world, const char *cache_dir, char **log);
void drs_slab_plan(const drs_slab *s, long out[8]);   /* lo, hi, z0, z1, Lloc, G, H, every */
int drs_slab_connect(drs_slab *s, const void *id128, void *main_stream /* hipStream_t or NULL: own stream */);
int drs_slab_run(drs_slab *s, void *d_a, void *d_b, int iterations /* < 0: the spec's */);
int drs_slab_sync(drs_slab *s);
void *drs_slab_stream(drs_slab *s);
const char *drs_slab_info(drs_slab *s);     /* JSON */
const char *drs_slab_error(const drs_slab *s);
void drs_slab_close(drs_slab *s);

/* ---- inputs and error metric: common.hpp:9-102 (host memory) */
void drs_fill_random_f64(double *a, size_t n, unsigned seed);   /* seed 1 == the reference's unseeded rand() */
void drs_fill_random_f32(float *a, size_t n, unsigned seed);
double drs_check_error_f64(int ndim, int L, int M, int N, int halo, const double *out, const double *ref,
                           double *max_abs, long *max_idx, double *max_rel);
double drs_check_error_f32(int ndim, int L, int M, int N, int halo, const float *out, const float *ref,
                           double *max_abs, long *max_idx, double *max_rel);

const char *drs_version(void);

#ifdef __cplusplus
}
#endif
#endif
