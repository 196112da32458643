// schedule.hpp -- the schedule analysis: everything the generator decides about a kernel after the planner has fixed its
// geometry, as a value.  Built from the finished plan and the options, both const; it emits no text.  It holds
//   * the window analysis (which elements of the arriving plane a lane reads from LDS, when, and how they group into vectors)
//     and the coefficient table of --coef sgpr;
//   * the predicates of the reuse schedule and of the emission (carry, scatter, rotmod, pin, packed, skewed, bufstore, ...);
//   * the numbers that follow from them: LDS slots, prefetch depth, unroll of the streaming loop, the LDS row length in whole vectors, the LDS
//     image and its size, the halo-loader task counts, the workgroup -> tile map and the grid size, the register demand the tuner filters on and
//     the recommended placement of the output array; and config_error(): what the schedule cannot do with this plan.
// generator.hpp asks it whether the configuration is valid, emit_hip.hpp turns it into the kernel, emit_host.hpp publishes it
// (info JSON, host programs).  Data flows one way: plan + options -> Schedule -> text.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "plan.hpp"

namespace drs {

inline std::string sfmt(const char *fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

inline int pmod(int a, int m) { return ((a % m) + m) % m; }
inline int lcm_i(int a, int b) { int x = a, y = b; while (y) { int t = x % y; x = y; y = t; } return a / x * b; }

struct Schedule {
    Schedule(const KernelPlan &plan, const GenOptions &opt) : p(plan), o(opt), xcd_remap(opt.xcd_remap), SROW(round_up(plan.SROW_MIN, plan.VL)) {
        // auto mapping: 3D sweeps use one x-y band per XCD when a plane has enough tiles to
        // balance 8 bands, else a contiguous chunk per XCD; one-shot 2D tiles and 2D row
        // streams keep the dispatch order (a single linear front, best measured)
        if (xcd_remap < 0) xcd_remap = (p.ndim == 3 && p.stages == 1) ? ((p.NBX * p.NBY >= 64) ? 2 : 1) : 0;
        analyse();
    }
    const KernelPlan &p;
    const GenOptions &o;
    int xcd_remap;           // --xcd-remap with the automatic choice resolved
    int SROW;                // LDS row length, whole vectors
    int NSLOT = 2;           // LDS plane slots
    int PD = 1;              // prefetch depth (planes in flight)
    int UN = 1;              // unroll of the streaming loop

    long lds_bytes_for(int nslot) const { return (long)nslot * p.SROWS * SROW * esize(); }
    long lds_elems() const {
        if (skew_db()) return (long)p.SROWS * SROW + 2L * (p.stages - 1) * cslot() + p.TX + 2 * p.VL;      // source slot + double-buffered compact slots + a guard row
        return p.dma ? dma_lo() + (long)NSLOT * dma_slot() + dma_hi() : (long)NSLOT * p.SROWS * SROW;
    }
    long lds_bytes() const { return lds_elems() * esize(); }

    // ---- window analysis -------------------------------------------------------------
    struct Elem {
        int dr, dc;
        bool own = false;
        int r = 0, q = 0, e = 0;      // own: row, vector, element
        int first = 0;                // earliest age of its plane (iterations since arrival) at which it is read from LDS; 0 = on arrival
        std::set<int> ages;           // every age at which it is (re)read from LDS
        std::set<int> uses;           // ages at which a tap reads it
        int vec = -1, ve = 0;         // member of rim vector `vec`, element ve
        int sc = -1;                  // rim scalar id
    };
    struct RimVec { int dr, c0, first; std::set<int> ages; };
    std::map<std::pair<int, int>, Elem> U;
    std::vector<RimVec> rimvecs;
    std::vector<std::pair<int, int>> rimscalars;  // (dr,dc) by id
    int max_first = 0;    // oldest age at which any rim element is still read from LDS (that many extra LDS plane slots stay live)
    bool bufstore() const { return o.store_mask == "buffer"; }
    // plane loads through a window that closes past the block's last plane (--uniform-loads 2): streaming kernels with
    // prefetch whose plane fits a 31-bit byte offset
    bool bufload() const { return o.uniform_loads == 2 && p.has_s && p.prefetch && o.clamp_loads && (double)p.stride_s * esize() < 2.0e9; }
    // 32-bit registers of the per-lane state the kernel names: partial sums, register windows (own points + rims) and the
    // prefetch sets.  The tuner's FilterParams compares it with the register file a lane can have at the workgroup's size
    // (drstencil_amd/tuner/tuning.py: fitted against the compiler's resource reports, profiles/r02_reg_model.md).
    int reg_demand() const { return reg_demand_sweep() + (p.fp32 ? 1 : 2) * (extra_streams() * old_sets() * p.RY * p.VX + residual_words() + coef_words()); }
    // ---- --varcoef: tap t's coefficient at every cell the lane stores is one more stream of that kind per tap, from grid t of coef
    // (kv<t>_0_<r>_<q>), under the store's guards -- but with a plane lead of its own and at distance 0: in iteration u the arriving source
    // plane adds its taps of streamed offset ds to output plane k + u + (zh - ds), so tap t's values are loaded zh - t.ds planes ahead of the
    // plane pout points at, in front of the iteration's barrier, and meet their FMAs behind it.  One set: T * RY * VX elements live across
    // the barrier (they do not join extra_streams(): the other streams keep their distance and their sets).  The prologue iterations load
    // theirs the same way, from the block's first planes.
    int coef_words() const { return p.varcoef ? (int)p.taps.size() * p.RY * p.VX : 0; }
    // ---- --time-order 2: the old output, the sweep's third memory stream -----------------------------------------------------------
    // out = S(in) - out_old.  The old vector of every (r, q) the lane stores is loaded into named registers ov<set>_<r>_<q>, under the
    // store's own guards, old_dist() planes AHEAD of the iteration that completes and stores that plane: with --prefetch at the prefetch
    // distance, next to the source-plane loads (its latency runs under PD planes of LDS exchange, barriers and FMAs), else at the top of
    // the plane's own iteration, in front of the LDS write and the barrier.  The sets rotate by renaming (the unroll is a multiple of
    // PD + 1).  The value is read once: a non-temporal load.  emit_final subtracts it from the finished sums in place.
    // ---- --source: the source term is one more stream of the same kind, from a third array: out = S(in) + src, or (S(in) - out_old) + src.
    // Both extra read streams share the distance and each has its own family of old_dist() + 1 register sets (sv<set>_<r>_<q> beside ov...).
    // ---- --residual max: the centre value is a third stream of that kind, from `in` itself: the input's value at every cell the lane stores
    // (cv<set>_<r>_<q>), same guards, same distance, same number of sets -- but ordinary cached loads (the workgroup fetched these lines a few
    // planes earlier) and nothing is applied to the sums: emit_final folds |sum - centre| of every stored element into the lane's running
    // maximum rmax.  At every exit of the kernel the workgroup reduces its lanes' maxima (cross-lane inside a wavefront, one value per
    // wavefront through the LDS image, which is free by then) and writes ONE partial, d_res[1 + blockIdx.x]; res_<name> folds them.
    // ---- --dirichlet: fix is a fourth stream of that kind, from its own array: out = fix where fix is not NaN.  It joins the count: the
    // same distance, its own family of register sets (fv<set>_<r>_<q>), and emit_final selects with it after the other two are applied.
    // ---- --scale: w is a fifth stream of that kind, from its own array: v = w * S(in), applied first (wv<set>_<r>_<q>).  --scale-centre c
    // makes the centre sets live exactly as --residual does (v = C * in + w * S(in)); with both options there is ONE family of centre
    // sets, loaded once, and residual_words() counts it once.
    int extra_streams() const { return (p.second_order ? 1 : 0) + (p.source ? 1 : 0) + (p.dirichlet ? 1 : 0) + (p.scale ? 1 : 0); }
    int old_dist() const { return ((extra_streams() || p.residual) && p.prefetch && p.has_s && !p.dma) ? PD : 0; }
    int old_sets() const { return old_dist() + 1; }
    int residual_words() const { return (p.centre_live() ? old_sets() * p.RY * p.VX : 0) + (p.residual ? 1 : 0); }      // elements: the centre sets (--residual, --scale-centre: one family) and rmax
    long residual_elems() const { return p.residual ? 1L + grid_size() : 0L; }                // d_res: the result, then one partial per launched workgroup
    int reg_demand_sweep() const {
        const int words = p.fp32 ? 1 : 2, pts = p.RY * p.VX;
        const int stg = (p.prefetch && p.has_s ? PD + 1 : 1) * (pts + hl_iters() * p.VL);   // the staged plane and the prefetch sets
        if (p.stages > 1 && pin()) {
            // pinned pipelines (round 4): per stage Range - 1 sums live across iterations plus one in the making; the lane's own points of every
            // stage; ONE stage's rim at a time; the prefetch sets.  (Allocated: 126 for 120 named on the 3-stage, 151 for 144 on the 4-stage fp64 kernel.)
            const int rim = (int)rimvecs.size() * p.VL + (int)rimscalars.size();
            return words * ((p.stages * (range() - 1) + 1) * pts + p.stages * pts + (rows_order() ? p.VX + p.hxm + p.hxp : rim) + stg);
        }
        const int sums = scatter() ? p.stages * rotmod() * pts : (carry() + 1) * pts;
        if (rows_order()) {
            // the plane is consumed row by row: one row of window (own vector + x neighbours, twice when odd pairs are assembled)
            // for the group at work and the next row's vector already requested
            const int rowwin = (p.VX + p.hxm + p.hxp) * (packed() ? 2 : 1) + p.VX;
            return words * (sums + p.stages * pts + rowwin + stg);
        }
        const int window = p.RY * p.VX + (int)rimvecs.size() * p.VL + (int)rimscalars.size();
        const int windows = (scatter() ? p.stages : resident_planes()) * window;
        return words * (sums + windows + (p.dma ? 0 : stg));
    }
    // ---- LDS image of --stage dma --------------------------------------------------------------------------------------
    // One wavefront instruction of LDS-DMA writes its 64 lanes' 16 bytes to consecutive LDS addresses, so a plane slot is
    //   own region : [row r][vector q][lane tid] of vec_t  -- instruction (r, q) of wave w fills 64 consecutive vectors
    //   halo region: [loader task] of vec_t                 -- x-halo pieces [piece][tile row], then y-halo rows [row][piece]
    // instead of the row-major tile with pad columns of the register-staged path.  A window element (dr, dc) of a lane lives
    // at sbt + K(dr, dc) in the own region (K a compile-time constant: the owner is lane tid + a*BX + c) unless it falls off
    // the tile, where the edge lanes re-read it from the halo region under the tile-edge branches (emit_reads_dma).
    long dma_own() const { return (long)p.NT * p.RY * p.NV * p.VL; }
    long dma_slot() const { return dma_own() + (long)hl_iters() * p.NT * p.VL; }
    long dma_kown(int dr, int dc) const {
        const int a = fdiv(dr, p.RY), b = dr - a * p.RY, c = fdiv(dc, p.VX), v = dc - c * p.VX;
        return ((long)(b * p.NV + v / p.VL) * p.NT + (long)a * p.BX + c) * p.VL + v % p.VL;
    }
    // guard elements in front of the first and behind the last slot: edge lanes compute own-region addresses of lanes that do
    // not exist (their values are replaced under the edge branches); the addresses must still lie inside the allocation
    long dma_lo() const { return round_up((int)std::max(0L, -dma_kown(-p.hym, -p.hxm)) + p.VL, p.VL); }
    long dma_hi() const { return round_up((int)(((long)fdiv(p.RY - 1 + p.hyp, p.RY) * p.BX + fdiv(p.VX - 1 + p.hxp, p.VX) + 2) * p.VL), p.VL); }
    int dma_rows() const { return tile_rows(); }
    long dma_xh_base() const { return dma_own(); }                                   // x-halo pieces: task id = piece * rows + row
    long dma_yh_base() const { return dma_own() + (long)xtasks() * p.VL; }           // y-halo rows: task id = xtasks + row * pieces + piece
    long dma_srowh() const { return (long)row_pieces() * p.VL; }
    int esize() const { return p.fp32 ? 4 : 8; }
    int rowpos(int r) const { return p.cyclic_y ? r * p.BY : r; }
    // --cyclic-merge-x (reference: for_declare, codegen.hpp:116-141, `mi += blockDim.x`): a lane's points are Bx columns apart -- one
    // 4/8-byte access per lane and point, 64 lanes x one element = one contiguous run per wavefront instruction -- instead of contiguous
    int colpos(int v) const { return p.cyclic_x ? v * p.BX : v; }
    long own_off(int r, int q) const { return (long)rowpos(r) * p.stride_y + (long)colpos(q * p.VL); }   // vector q of row r, elements from the lane's first point
    static int fdiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
    // ---- the reuse schedule (reference: forward/backward partition, drstencil.hpp:198-259) ------------------------------------
    // R = zh - zl + 1 source planes contribute to an output plane.  The reference keeps `Range` planes in shared memory and
    // moves the rest of the reuse through partial sums (`out[k+Dist] = forward_k`, atomicAdd of the backward set,
    // codegen.hpp:385-428).  Here: W = resident_planes() source planes live in register windows, and a partial sum is CARRIED in
    // VGPRs for carry() = R - W iterations: an output plane's sum is started when plane (zh - carry) of its stencil arrives, with
    // the taps of the older planes read from the retained windows in gold order, and receives one group of taps per arriving
    // plane from then on.  carry = R-1 is --schedule scatter (nothing retained), carry = 0 is --schedule window (nothing
    // carried); --schedule reuse takes W from the reference's own Range for the given --dist.  Results never depend on it.
    int carry() const {
        const int R = p.zh - p.zl + 1;
        if (o.schedule == "window") return 0;
        if (o.schedule == "reuse") return R - std::max(1, std::min(R, p.range));
        return R - 1;
    }
    int resident_planes() const { return (p.zh - p.zl + 1) - carry(); }
    bool scatter() const { return p.stages > 1 || !p.has_s || carry() == p.zh - p.zl; }
    // ---- --order rows (round 3): the emitter bounds live ranges itself ---------------------------------------------------------------
    bool rows_order() const { return o.order == "rows"; }
    bool skewed() const { return (o.skew > 0 || (o.skew < 0 && p.stages >= 3)) && p.stages > 1 && p.has_s && p.prefetch && !p.dma; }
    // --skew 2: the intermediate planes' slots are double-buffered by iteration parity, so a stage writes its completed plane to its
    // consumer's slot as soon as it has it -- inside the compute phase, under the other wavefronts' FMAs -- instead of in a burst of LDS
    // writes between the iteration's two barriers; only the source plane's staging stays there.  The extra slots are COMPACT (tile rows
    // x tile columns, no pad columns, no halo rows: an intermediate plane has no halo; edge lanes read a neighbouring row / slot instead,
    // values that only reach outputs the tile does not own): fp64 132 x 30 tiles, 3 stages: 34.8 KB + 4 x 31.7 KB = 158 of the 160 KiB.
    bool skew_db() const { return skewed() && o.skew >= 2; }
    long cslot() const { return (long)(p.has_y ? p.TY : 1) * p.TX; }
    // two adjacent x points per v_pk_fma_f32: fp32, vectors of 2 or 4 elements (a pair is a half of an accumulator vector)
    // Rotation by renaming: the partial sums of the planes in flight cycle through `rotmod()` register sets, and the streaming loop is
    // unrolled by lcm(rotmod, LDS slots, prefetch sets).  rotmod = Range is the minimum; --rot-mod m >= Range adds m - Range idle
    // sets (points-per-lane registers each) and can shrink the unroll a lot: Range 7 with 2 LDS slots and 2 prefetch sets unrolls
    // 14 plane bodies, --rot-mod 8 unrolls 8.  A fused 63-tap body is ~5 KB of FMAs: 14 of them exceed the 64 KB instruction
    // cache that two CUs share, 8 fit (profiles/r03_exp_r3c.log).
    int rotmod() const { const int R = p.zh - p.zl + 1; return (rot_mod_ > R && scatter()) ? rot_mod_ : R; }
    int rot_mod_ = 0;
    // auto: with --order rows, and for pipelines of three or more stages (their nine planes of sums do not survive the compiler's sinking: the
    // unpinned fp64 3-stage kernel needs scratch at 990 lanes, the pinned one 124-126 VGPRs)
    bool pin() const { return o.pin < 0 ? (rows_order() || p.stages >= 3) : o.pin != 0; }
    bool packed() const { return rows_order() && p.fp32 && (p.VL == 2 || p.VL == 4) && o.pack != 0; }
    // --coef sgpr: the stencil's distinct coefficient values live in scalar registers (one s_mov each at kernel entry, made opaque by an
    // empty asm) instead of being 32-bit literals of every FMA: `v_fmac_f32 v, s, v` is a 4-byte VOP2 where `v_fmac_f32 v, 0x3cc49ba6, v`
    // takes 8 -- the fused 63-tap fp32 kernel is 56 KB of code otherwise, and two CUs share one 64 KB instruction cache and its fetch
    // bandwidth.  fp32 only (an fp64 FMA is VOP3 and takes its coefficient from a scalar pair already); at most 24 values (scalar registers).
    bool coef_sgpr() const { return p.fp32 && o.coef_sgpr > 0 && !coef_idx_.empty(); }
    std::map<std::string, int> coef_idx_;     // coefficient as printed -> index of its scalar constant kc<i>
    // ---- placement of the output array (round 3, scripts/archive/probe_skew*.py) ----------------------------------------------------------------
    // Launch time of a z-streaming kernel depends on (out - in) mod 64 MiB: all resident workgroups read plane k + zh + PD while they write
    // plane k; when the written addresses fall, modulo 64 MiB, 8-16 MiB BEHIND the read front (planes read moments ago, which neighbouring
    // tiles' halo re-reads still want from the memory-side cache), the 1024^3 step-2 kernel takes 1.65-1.68 ms instead of 1.46-1.48
    // (profiles/r03_probe_skew4.log: period exactly 64 MiB, forward launch bad for delta in [4, 12] MiB, the reverse launch of the
    // ping-pong for [52, 60]).  The ping-pong runs both directions, so the skew is the point of {0, 32 MiB} farther from both windows.
    // Kernels with several z fronts in flight (short stream blocks) or small planes (< 2 MiB) are flat: skew 0.
    static constexpr long kPlacementPeriod = 64L << 20;
    long out_skew_bytes() const {
        if (o.out_skew >= 0) return ((long)o.out_skew << 20) % kPlacementPeriod;
        const long plane = p.stride_s * (long)esize();
        if (p.ndim != 3 || !p.has_s || plane < (2L << 20)) return 0;
        const long ahead = (long)(p.stages * p.zh + (p.prefetch ? PD : 0) + (skewed() ? p.stages - 1 : 0)) * plane;       // read front - write front (a skewed pipeline's stages lag one more plane each)
        const long c = (((ahead - (12L << 20)) % kPlacementPeriod) + kPlacementPeriod) % kPlacementPeriod;   // centre of the forward launch's bad window
        const long d0 = std::min(c, kPlacementPeriod - c);                                  // distance of skew 0 from the windows at +-c
        const long d32 = std::labs(c - (32L << 20));                                        // ... of skew 32 MiB
        return d32 >= d0 ? (32L << 20) : 0;
    }
    std::string cfg_error_;
    const std::string &config_error() const { return cfg_error_; }
    // iterations after its arrival at which the taps with streamed offset ds read their plane
    int age_of(int ds) const { return std::max(0, p.zh - carry() - ds); }

    void analyse() {
        {   // --coef sgpr: the most frequent coefficient values first, 24 at most
            std::map<std::string, int> freq;
            for (auto &t : p.taps) freq[t.coef]++;
            std::vector<std::pair<int, std::string>> byf;
            for (auto &kv : freq) byf.push_back({-kv.second, kv.first});
            std::sort(byf.begin(), byf.end());
            for (size_t i = 0; i < byf.size() && i < 24; i++) coef_idx_[byf[i].second] = (int)i;
        }
        // own elements
        for (int r = 0; r < p.RY; r++)
            for (int v = 0; v < p.VX; v++) {
                Elem e; e.dr = rowpos(r); e.dc = colpos(v); e.own = true; e.r = r; e.q = v / p.VL; e.e = v % p.VL; e.first = 0;
                U[{e.dr, e.dc}] = e;
            }
        // needed elements, with the ages at which their taps run
        const bool hybrid = !scatter();
        for (auto &t : p.taps)
            for (int r = 0; r < p.RY; r++)
                for (int v = 0; v < p.VX; v++) {
                    std::pair<int, int> key{rowpos(r) + t.dy, colpos(v) + t.dx};
                    auto it = U.find(key);
                    if (it == U.end()) { Elem e; e.dr = key.first; e.dc = key.second; it = U.insert({key, e}).first; }
                    it->second.uses.insert(hybrid ? age_of(t.ds) : 0);
                }
        // When is a rim element read from its plane's LDS slot?  On its first use, and then it is either kept in its register
        // until its later uses ("carried") or read again when they are due ("folded into the window read": the register is free
        // in between, the LDS slot stays live that much longer).
        //   --schedule window: --lazy-rims 1 reads on first use, 0 on arrival; always kept afterwards.
        //   --schedule reuse: like the reference's --merge-forward (drstencil.hpp:248-256: a forward set smaller than the
        //   threshold is folded back), per retained plane: fewer in-plane taps on that plane than --merge-forward -> its elements
        //   are read again when that plane's taps run, else they are carried from their first read.
        std::map<int, int> inplane_taps;     // age -> taps that leave the lane's own points
        for (auto &t : p.taps) if (t.dy != 0 || t.dx != 0) inplane_taps[hybrid ? age_of(t.ds) : 0]++;
        for (auto &kv : U) {
            Elem &e = kv.second;
            if (e.own) { e.ages = {0}; continue; }
            const int first_use = *e.uses.begin();
            if (!hybrid || (o.schedule == "window" && !o.lazy_rims)) { e.ages = {0}; continue; }
            e.ages = {first_use};
            if (o.schedule == "reuse")
                for (int a : e.uses) if (a > first_use && inplane_taps[a] < o.merge_forward) e.ages.insert(a);
        }
        // group the non-own elements of a row into whole aligned vectors where possible
        std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> chunks;  // (dr, chunk) -> keys
        for (auto &kv : U) if (!kv.second.own) chunks[{kv.second.dr, fdiv(kv.second.dc, p.VL)}].push_back(kv.first);
        for (auto &c : chunks) {
            if ((int)c.second.size() == p.VL && p.VL > 1) {
                RimVec rv; rv.dr = c.first.first; rv.c0 = c.first.second * p.VL;
                for (auto &key : c.second) rv.ages.insert(U[key].ages.begin(), U[key].ages.end());
                rv.first = *rv.ages.begin();
                for (auto &key : c.second) { U[key].vec = (int)rimvecs.size(); U[key].ve = U[key].dc - rv.c0; U[key].ages = rv.ages; }
                rimvecs.push_back(rv);
            } else {
                for (auto &key : c.second) { U[key].sc = (int)rimscalars.size(); rimscalars.push_back(key); }
            }
        }
        for (auto &kv : U) kv.second.first = *kv.second.ages.begin();
        max_first = 0;
        for (auto &kv : U) if (!kv.second.own) max_first = std::max(max_first, *kv.second.ages.rbegin());
        NSLOT = p.has_s ? max_first + 2 : 1;
        // temporal blocking: stage t exchanges through LDS plane t % NSLOT, one barrier per stage;
        // two planes suffice for an even number of stages, three for an odd one
        if (p.stages > 1) NSLOT = (p.stages % 2 == 0) ? 2 : 3;
        // --skew: every stage owns one slot (read between the iteration's two barriers, rewritten after the second)
        if (skewed()) NSLOT = p.stages;
        // deeper prefetch rotates PD+1 register sets; one more LDS plane keeps the unroll at lcm(range, PD+1)
        {
            const bool fused3d = p.ndim == 3 && p.stages == 1 && p.step > 1;
            const bool light = p.gtaps.size() <= 25;    // heavier fused stencils have no registers to spare for extra sets
            // (rows order: depth 1 -- a second prefetch set lifts the fused step-3 kernel over 128 VGPRs, i.e. to one workgroup per CU: 1.65 -> 2.26 ms)
            int want = o.prefetch_depth < 0 ? (fused3d && light && !o.ref_defaults && !rows_order() ? (p.fp32 ? 3 : 2) : 1) : o.prefetch_depth;   // fp64 depth 3: -20 % (VGPRs)
            PD = (p.prefetch && p.has_s) ? std::max(1, std::min(6, want)) : 1;
            const int nslot0 = NSLOT;
            if (PD > 1 && p.stages == 1 && NSLOT < PD + 1 && (PD + 1) % NSLOT != 0) NSLOT = PD + 1;
            // the automatic choice never costs a configuration its LDS budget
            if (o.prefetch_depth < 0 && PD > 1 && lds_bytes_for(NSLOT) > 64 * 1024) { PD = 1; NSLOT = nslot0; }
        }
        if (p.ws) {
            // wave specialisation: the loader wavefronts keep PD planes in flight into a ring of PD + 1 LDS slots
            PD = o.prefetch_depth < 0 ? 3 : std::max(1, std::min(6, o.prefetch_depth));
            NSLOT = PD + 1;
        }
        UN = 1;
        if (p.has_s) {
            // rotation by renaming: partial-sum sets (carry + 1), register windows, LDS slots and prefetch sets all return to
            // their starting names after one trip of the unrolled loop
            const int nsets = p.prefetch ? PD + 1 : 1;
            rot_mod_ = o.rot_mod;
            if (o.rot_mod == 0 && rows_order() && scatter() && p.stages == 1) {
                // automatic with --order rows: the modulus in [Range, Range + 3] with the shortest unrolled loop (one set of sums costs
                // points-per-lane registers, which pinned kernels can afford; rounds 1-2 kernels keep Range)
                const int R0 = p.zh - p.zl + 1;
                int best = R0;
                for (int m = R0; m <= R0 + 3; m++)
                    if (lcm_i(lcm_i(m, NSLOT), nsets) < lcm_i(lcm_i(best, NSLOT), nsets)) best = m;
                rot_mod_ = best;
            }
            const int rot = scatter() ? rotmod() : lcm_i(carry() + 1, resident_planes());
            UN = skewed() ? lcm_i(lcm_i(rot, nsets), skew_db() ? 2 : 1) : lcm_i(lcm_i(rot, NSLOT), nsets);     // skewed: the slots do not rotate (--skew 2: they alternate)
            const int base_un = UN;
            while (UN < o.stream_unroll && UN < 16) UN += base_un;
        }
        if (p.residual && lds_elems() < ceil_div(p.NT, 64)) cfg_error_ = "--residual: the LDS image holds fewer elements than the workgroup has wavefronts";
        if (o.skew > 0 && p.stages > 1 && !skewed()) cfg_error_ = "--skew 1 needs a streaming temporal pipeline with --prefetch (register staging)";
        if (rows_order()) {
            if (!scatter()) cfg_error_ = "--order rows needs the scatter schedule (every partial sum carried)";
            else if (p.cyclic_y) cfg_error_ = "--order rows needs block y merging";
            else if (p.cyclic_x) cfg_error_ = "--order rows needs block x merging";
            else if (p.dma) cfg_error_ = "--order rows stages planes through registers (--stage reg)";
            else if (o.debug_skip) cfg_error_ = "--debug-skip is not available with --order rows";
        }
    }

    int range() const { return p.zh - p.zl + 1; }
    int nwg() const { return p.NBX * p.NBY * p.NBS; }
    int band() const { return ceil_div(p.NBX * p.NBY, 8); }   // x-y tiles per XCD band (xcd-remap 2)
    int zgroup() const { return std::max(1, std::min(o.zgroup, p.NBS)); }
    // --xcd-remap 4: work units of `unit_tiles()` consecutive x-y tiles of ONE stream block (32 = the CUs of an XCD: whole tile rows when a
    // row has 8 tiles), dealt round-robin to the XCDs.  An XCD's 32 CUs start a unit's workgroups together and they stay in step (same
    // length, same code), so the halo rows / columns two neighbouring tiles of the unit both read are fetched from HBM once and hit
    // the XCD's L2 the second time -- what overlapped tiles (temporal pipelines) need most.
    int unit_tiles() const { return 32; }
    int units_per_block() const { return ceil_div(p.NBX * p.NBY, unit_tiles()); }
    int xcd_chunk() const { return std::max(1, o.xcd_chunk); }
    int grid_size() const {
        if (xcd_remap == 5) return round_up(nwg(), 8 * xcd_chunk());
        if (xcd_remap == 4) return 8 * unit_tiles() * ceil_div(units_per_block() * p.NBS, 8);
        if (xcd_remap == 3) return 8 * band() * zgroup() * ceil_div(p.NBS, zgroup());
        return xcd_remap == 2 ? 8 * band() * p.NBS : round_up(nwg(), 8);
    }

    // ---- staging of one plane ------------------------------------------------------------
    // halo-loader tasks per plane
    int nl() const { return p.PADL / p.VL; }
    int nr() const { return p.PADR / p.VL; }
    int tile_rows() const { return p.has_y ? p.TY : 1; }
    // halo loader tasks per plane: x halo pieces of every tile row, then whole y halo rows
    int xtasks() const { return ((o.debug_skip & 1) || !p.exact_x) ? 0 : tile_rows() * (nl() + nr()); }
    int row_pieces() const { return (p.PADL + p.TX + p.PADR) / p.VL; }
    int ytasks() const { return (p.has_y && p.exact_y && !(o.debug_skip & 2)) ? (p.hym + p.hyp) * row_pieces() : 0; }
    int halo_tasks() const { return xtasks() + ytasks(); }
    int hl_iters() const { return halo_tasks() ? ceil_div(halo_tasks(), p.NT) : 0; }   // rounds of tasks: one vector access per lane and round
};

}  // namespace drs
